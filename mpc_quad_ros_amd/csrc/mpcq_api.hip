// mpcq_api.hip — C ABI (include/mpcq.h) over the HIP kernels in mpcq_kernels.hpp.
// Host side of the engine: device allocations, precision dispatch, launches on a private
// stream, HIP-event timing, optional RCCL reduction of the swarm statistics.
// Device memory has two kinds of owner and no other: the arrays of fixed size register with the engine as they are allocated
// (EngineT::dalloc -> mpcq_engine::arrays), scratch that is sized by a request is a DevBuf.  Kernel argument structs hold raw pointers and own nothing.
#include <hip/hip_runtime.h>
#include <dlfcn.h>

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#define MPCQ_BUILDING_LIBRARY
#ifndef MPCQ_AUTO_GROUPS   // groups of mpcq_sim_steps for a streaming batch when tune.groups = 0 (see EngineT::init)
#define MPCQ_AUTO_GROUPS 2
#endif
#include "../../include/mpcq.h"
#include "mpcq_kernels.hpp"
#include "mpcq_replan.hpp"
#include "mpcq_circle.hpp"
#include "mpcq_replan_nl.hpp"
#include "mpcq_mission.hpp"
#include "mpcq_record.hpp"
#include "mpcq_blackbox.hpp"
#include "mpcq_explore.hpp"
#include "mpcq_score.hpp"
#include "mpcq_predict.hpp"
#include "mpcq_train.hpp"
#include "mpcq_fleet.hpp"
#include "mpcq_sensor.hpp"

namespace mpcq {   // mpcq_spec.hip, one translation unit per specialised shape
template <typename T> using StepFn = void (*)(const DevModel<T>, const DevState<T>, const int);
#if defined(MPCQ_SHAPE_LIST)   // reproducer builds (tools/repro_codegen): -D'MPCQ_SHAPE_LIST(X)=X(20,10) X(20,20)'
#define MPCQ_SPEC_SHAPES(X) MPCQ_SHAPE_LIST(X)
#elif defined(MPCQ_CHECKED) || defined(MPCQ_ONE_SHAPE)   // the checked build compiles for tens of minutes per specialised shape: only the headline shape has one there (MPCQ_ONE_SHAPE: quick A/B variants, `make variant SHAPES=20_10 EXTRA=-DMPCQ_ONE_SHAPE`)
#ifndef MPCQ_ONE_N
#define MPCQ_ONE_N 20
#define MPCQ_ONE_NB 10
#endif
#define MPCQ_SPEC_SHAPES(X) X(MPCQ_ONE_N, MPCQ_ONE_NB)
#else
#define MPCQ_SPEC_SHAPES(X) X(20, 10) X(20, 20) X(50, 50)   // BASELINE configs[1] (and [3] per rank), configs[2], configs[4]
#endif
// (one more macro level so that shapes given as macros -- MPCQ_ONE_N -- are expanded before the names are pasted)
#define MPCQ_DECL_(n, nb) StepFn<double> spec_lock_f64_##n##_##nb(int layout); StepFn<float> spec_lock_f32_##n##_##nb(int layout);
#define MPCQ_DECL(n, nb) MPCQ_DECL_(n, nb)
MPCQ_SPEC_SHAPES(MPCQ_DECL)
#undef MPCQ_DECL
// specialised free-running instances: the shapes of MPCQ_SPEC_RUN_SHAPES (Makefile: SPEC_RUN_SHAPES; reproducer builds: every shape)
#if defined(MPCQ_SPEC_RUN) && !defined(MPCQ_SPEC_RUN_SHAPES)
#define MPCQ_SPEC_RUN_SHAPES(X) MPCQ_SPEC_SHAPES(X)
#endif
#ifdef MPCQ_SPEC_RUN_SHAPES
#define MPCQ_DECLR_(n, nb) StepFn<double> spec_run_f64_##n##_##nb(int layout); StepFn<float> spec_run_f32_##n##_##nb(int layout);
#define MPCQ_DECLR(n, nb) MPCQ_DECLR_(n, nb)
MPCQ_SPEC_RUN_SHAPES(MPCQ_DECLR)
#endif
}
#define MPCQ_TRY64_(n, nb_) if (N == n && nb == nb_) return mpcq::spec_lock_f64_##n##_##nb_(layout);
#define MPCQ_TRY32_(n, nb_) if (N == n && nb == nb_) return mpcq::spec_lock_f32_##n##_##nb_(layout);
#define MPCQ_TRY64(n, nb_) MPCQ_TRY64_(n, nb_)
#define MPCQ_TRY32(n, nb_) MPCQ_TRY32_(n, nb_)
static mpcq::StepFn<double> spec_step(int N, int nb, int layout, double*) {   // lockstep instance of a specialised shape (layout: lds_layout), or nullptr
  MPCQ_SPEC_SHAPES(MPCQ_TRY64)
  return nullptr;
}
static mpcq::StepFn<float> spec_step(int N, int nb, int layout, float*) {
  MPCQ_SPEC_SHAPES(MPCQ_TRY32)
  return nullptr;
}
#ifdef MPCQ_SPEC_RUN_SHAPES
#define MPCQ_TRYR_(n, nb_) if (N == n && nb == nb_) return mpcq::spec_run_f64_##n##_##nb_(layout);
#define MPCQ_TRYR(n, nb_) MPCQ_TRYR_(n, nb_)
static mpcq::StepFn<double> spec_run(int N, int nb, int layout, double*) { MPCQ_SPEC_RUN_SHAPES(MPCQ_TRYR) return nullptr; }
#define MPCQ_TRYR32_(n, nb_) if (N == n && nb == nb_) return mpcq::spec_run_f32_##n##_##nb_(layout);
#define MPCQ_TRYR32(n, nb_) MPCQ_TRYR32_(n, nb_)
static mpcq::StepFn<float> spec_run(int N, int nb, int layout, float*) { MPCQ_SPEC_RUN_SHAPES(MPCQ_TRYR32) return nullptr; }
#endif

namespace {

thread_local std::string g_err;
int fail(int code, const std::string& msg) { g_err = msg; return code; }

#define HIP_TRY(expr)                                                                              \
  do {                                                                                             \
    hipError_t _e = (expr);                                                                        \
    if (_e != hipSuccess)                                                                          \
      return fail(MPCQ_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(_e));             \
  } while (0)

// ---- RCCL through dlopen (only loaded when a communicator is requested)
struct Id128 { char b[128]; };  // ncclUniqueId (passed by value)
struct Rccl {
  void* lib = nullptr;
  int (*GetUniqueId)(void*) = nullptr;
  int (*CommInitRank)(void**, int, Id128, int) = nullptr;
  int (*AllReduce)(const void*, void*, size_t, int, int, void*, hipStream_t) = nullptr;
  int (*CommDestroy)(void*) = nullptr;
  const char* (*GetErrorString)(int) = nullptr;
};
Rccl g_rccl;
int rccl_load() {
  if (g_rccl.lib) return 0;
  void* l = nullptr;
  if (const char* named = getenv("MPCQ_RCCL_LIB")) {   // another file than the system's RCCL (tests: a stand-in that reduces over shared memory)
    l = dlopen(named, RTLD_NOW | RTLD_GLOBAL);
    if (!l) return fail(MPCQ_ERR_COMM, std::string("dlopen MPCQ_RCCL_LIB: ") + dlerror());
  }
  if (!l) l = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
  if (!l) l = dlopen("/opt/rocm/lib/librccl.so", RTLD_NOW | RTLD_GLOBAL);
  if (!l) return fail(MPCQ_ERR_COMM, std::string("dlopen librccl.so: ") + dlerror());
  g_rccl.GetUniqueId = (int (*)(void*))dlsym(l, "ncclGetUniqueId");
  g_rccl.CommInitRank = (int (*)(void**, int, Id128, int))dlsym(l, "ncclCommInitRank");
  g_rccl.AllReduce = (int (*)(const void*, void*, size_t, int, int, void*, hipStream_t))dlsym(l, "ncclAllReduce");
  g_rccl.CommDestroy = (int (*)(void*))dlsym(l, "ncclCommDestroy");
  g_rccl.GetErrorString = (const char* (*)(int))dlsym(l, "ncclGetErrorString");
  if (!g_rccl.GetUniqueId || !g_rccl.CommInitRank || !g_rccl.AllReduce) return fail(MPCQ_ERR_COMM, "librccl.so lacks nccl symbols");
  g_rccl.lib = l;
  return 0;
}
constexpr int NCCL_FLOAT64 = 8, NCCL_SUM = 0, NCCL_MAX = 2;

// Every entry point runs with the engine's device current and restores the caller's afterwards (several engines on
// different devices in one process, calls from other host threads).
struct DeviceGuard {
  int prev = -1;
  bool switched = false;
  explicit DeviceGuard(int dev) {
    if (hipGetDevice(&prev) == hipSuccess && prev != dev) switched = hipSetDevice(dev) == hipSuccess;
  }
  ~DeviceGuard() { if (switched) (void)hipSetDevice(prev); }
};

// SPD inverse through Cholesky (K_x = K(X,X) + sn^2 I; np.linalg.inv in the reference, src/gp/RGP.py:157)
bool spd_inverse(const std::vector<double>& A, int n, std::vector<double>& Ai) {
  std::vector<double> G(A);
  for (int j = 0; j < n; ++j) {
    double d = G[j * n + j];
    for (int k = 0; k < j; ++k) d -= G[j * n + k] * G[j * n + k];
    if (!(d > 0)) return false;
    d = std::sqrt(d);
    G[j * n + j] = d;
    for (int i = j + 1; i < n; ++i) {
      double s = G[i * n + j];
      for (int k = 0; k < j; ++k) s -= G[i * n + k] * G[j * n + k];
      G[i * n + j] = s / d;
    }
  }
  std::vector<double> Gi(n * n, 0.0);
  for (int j = 0; j < n; ++j) {
    Gi[j * n + j] = 1.0 / G[j * n + j];
    for (int i = j + 1; i < n; ++i) {
      double s = 0;
      for (int k = j; k < i; ++k) s -= G[i * n + k] * Gi[k * n + j];
      Gi[i * n + j] = s / G[i * n + i];
    }
  }
  Ai.assign(n * n, 0.0);
  for (int a = 0; a < n; ++a)
    for (int b = 0; b <= a; ++b) {
      double s = 0;
      for (int k = a; k < n; ++k) s += Gi[k * n + a] * Gi[k * n + b];
      Ai[a * n + b] = Ai[b * n + a] = s;
    }
  return true;
}


// RGP constants of one axis (RGP.__init__, src/gp/RGP.py:140-157): K_x = K(X,X) + sn^2 I [nb][nb] and its inverse.  The routine behind
// mpcq_create and behind a caller's model in mpcq_rgp_train / mpcq_record_train.  false: K_x is not positive definite.
bool rgp_axis_constants(const double* X, int nb, double Lh, double sf, double sn, std::vector<double>& K, std::vector<double>& Ki) {
  K.assign((size_t)nb * nb, 0.0);
  for (int i = 0; i < nb; ++i)
    for (int j = 0; j < nb; ++j) {
      const double dl = X[i] - X[j];
      K[i * nb + j] = sf * sf * std::exp(-0.5 * dl * dl / (Lh * Lh)) + (i == j ? sn * sn : 0.0);
    }
  return spd_inverse(K, nb, Ki);
}

}  // namespace

// ------------------------------------------------------------------ engine
// The precision-independent view of an engine (mpcq_engine::view): what the side launches of a period and the trajectory-slot entry
// points (mpcq_replan, mpcq_replace_trajectories, mpcq_get_trajectories) work on.  Trajectories, cursors, the plant state, controls, costs
// and the solver's counters are float64 / int in every precision; only the RGP state and the step kernel's model are not, and stay EngineT's.
struct EngineView {
  double* traj; int* len; int* idx; int* finished; const double* plant; int Tmax;   // the trajectory slots and the plant state [B,13]
  const double* cost; const int* status; const int* qp_iter; const double* w;       // what the last step left: [B], [B], [B], [B,4]
  int N, skip;
  double g;
};
// Device scratch allocated on first use and replaced by a larger block when a request exceeds it (the contents are not kept).
// Move-only: declaring the move assignment deletes the copy operations.
template <typename P> struct DevBuf {
  P* p = nullptr;
  size_t elems = 0;
  DevBuf& operator=(DevBuf&& o) {
    release();
    p = o.p; elems = o.elems;
    o.p = nullptr; o.elems = 0;
    return *this;
  }
  ~DevBuf() { release(); }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr; elems = 0;
  }
  hipError_t grow(size_t need) {
    if (elems >= need) return hipSuccess;
    release();
    const hipError_t err = hipMalloc((void**)&p, need * sizeof(P));
    if (err == hipSuccess) elems = need;
    else p = nullptr;
    return err;
  }
};
// buf grown to `elems` elements, or MPCQ_ERR_DEVICE with `message` (the failed allocation's sticky HIP error is cleared: the caller's next
// HIP call must not meet it)
template <typename Buf> static int grow_or_fail(Buf& buf, size_t elems, const std::string& message) {
  if (buf.grow(elems) == hipSuccess) return 0;
  (void)hipGetLastError();
  return fail(MPCQ_ERR_DEVICE, message);
}

// ---- The per-period features.  Each hangs side launches behind the step kernel of every control period (EngineT::period) and is one
// section here: its state, the layout of its packed device buffers (written once, as accessors) and its launch over an EngineView.  The
// entry points of each stand in the C ABI part below, under the same heading.  What a period's side launches need to know about the period:
struct Tick {
  int row = -1;          // the recorder's row (-1: the period is not recorded)
  int bslot = -1;        // the black box's ring slot (-1: no black box)
  long long bper = -1;   // the black box's period number
  int mper = -1;        // the mission's period number (-1: no mission)
  long long sper = -1;   // the scoreboard's period number (-1: no score running)
  long long fper = -1;   // the fleet period of the plant update (-1: no fleet, or no plant update drawn)
  long long nper = -1;   // the sensor period of the measurement (-1: no sensor, or the period takes the caller's measurement)
};

// ---- flight recorder (mpcq_record_*, mpcq_record.hpp): host bookkeeping and device buffers of a recording; the launches depend on the
// precision (record_kernel<T> reads mu and C) and are EngineT's (rec_snapshot, rec_write).  The selection is kept sorted (a group of
// mpcq_sim_steps covers a contiguous part of it); pos maps the caller's order to it.
struct Recorder {
  bool on = false;
  int fields = 0, every = 1, capacity = 0, count = 0, rows = 0;
  long long dropped = 0, periods = 0;
  std::vector<int> sorted, pos;          // selection ascending; pos[j] = place of the caller's j-th quadrotor in `sorted`
  std::vector<int> glo, ghi;             // part of `sorted` inside entry g of mpcq_engine::groups: [glo[g], ghi[g])
  std::vector<long long> period_of;      // period number of every row
  DevBuf<int> d_sel;                     // sorted selection
  DevBuf<double> d_f[mpcq::record::NF - 1];   // double fields, [capacity][count][width]
  DevBuf<int> d_solver;                  // [capacity][count][4]
  DevBuf<double> d_snap;                 // [count][SNAP]: x_pred_prev and has_prev in front of the step (MPCQ_RECORD_DRAG)
  // A period (one fused step of every quadrotor) counts whether it is recorded or not; the row a recorded one writes (-1: not recorded --
  // no recording, not its turn, or the buffer is full and the period counts as dropped)
  int next_row() {
    if (!on) return -1;
    const long long p = periods++;
    if (p % every) return -1;
    if (rows >= capacity) { ++dropped; return -1; }
    period_of.push_back(p);
    return rows++;
  }
};

// ---- incident recorder (mpcq_blackbox_*, mpcq_blackbox.hpp): a ring of the recorder's rows per watched quadrotor and its trigger state on
// the device; the launches read the RGP state in the engine's precision and are EngineT's (bb_snapshot, bb_write).  The selection is kept
// sorted, as the recorder's is, and so are the rules and the per-quadrotor state; pos maps the caller's order to it.
struct BlackBox {
  bool on = false;
  int fields = 0, pre = 0, post = 0, D = 0, count = 0;
  long long periods = 0;                 // periods issued since mpcq_blackbox_start
  std::vector<int> sorted, pos;          // selection ascending; pos[j] = place of the caller's j-th quadrotor in `sorted`
  std::vector<int> glo, ghi;             // part of `sorted` inside entry g of mpcq_engine::groups: [glo[g], ghi[g])
  DevBuf<int> d_sel;                     // sorted selection
  DevBuf<mpcq_blackbox_rule> d_rules;    // [count], sorted order
  DevBuf<double> d_f[mpcq::record::NF - 1];   // double fields, [D][count][width]
  DevBuf<int> d_solver;                  // [D][count][4]
  DevBuf<double> d_snap;                 // [count][SNAP] (MPCQ_RECORD_DRAG)
  DevBuf<int> d_int;                     // ints(): state [count] | cause [count] | left [count]
  DevBuf<long long> d_i64;               // fired_period [count] | first [count]
  // read-out staging (mpcq_blackbox_get*): grown on demand
  DevBuf<double> d_stage;                // [n][D][width]
  DevBuf<int> d_stage_int;               // which [n] | rows [n] | solver rows [n][D][4]; the mask of a rearm [count]
  DevBuf<long long> d_stage_p0;          // [n]
  mpcq::blackbox::State state() const { return mpcq::blackbox::State{d_int.p, d_int.p + count, d_int.p + 2 * (size_t)count, d_i64.p, d_i64.p + count}; }
};

// ---- device missions (mpcq_mission_*, mpcq_mission.hpp): the queue of upcoming flights, the per-quadrotor leg counters and the log of
// consumed legs on the device, and what every flight is planned with.
struct Mission {
  bool on = false;
  int L = 0, n_wp = 0, order = 0, nonlinear = 0;
  double dt = 0;
  mpcq_nl::Opts opts;
  long long periods = 0;   // periods issued since mpcq_mission_set
  DevBuf<double> d_wp;     // [B,L,n_wp,3] (empty: no waypoint leg)
  DevBuf<mpcq_leg> d_legs; // [B,L]: kind, limits and radius of every leg
  DevBuf<double> d_info;   // [B,6] (nonlinear)
  DevBuf<int> d_int;       // ints(B)
  // The layout of d_int, and of the host image mission_begin fills (nl = B * L): leg [B] | installed [B] | last_code [B] | claim [B] |
  // leg_code [B,L] | leg_period [B,L]
  struct Ints { int *leg, *installed, *last_code, *claim, *leg_code, *leg_period; };
  static size_t n_ints(size_t B, size_t nl) { return 4 * B + 2 * nl; }
  static Ints ints_at(int* p, size_t B, size_t nl) { return Ints{p, p + B, p + 2 * B, p + 3 * B, p + 4 * B, p + 4 * B + nl}; }
  Ints ints(size_t B) const { return ints_at(d_int.p, B, B * (size_t)L); }
};
// The mission launch of one period (number `period` since mpcq_mission_set) for the quadrotors [b0, b0 + n) of B on stream s, behind
// everything the period has issued there.  start [B,13]: where the flights begin (the plant state behind its update, or the period's measurement).
static void mission_launch(const Mission& ms, const EngineView& t, size_t B, hipStream_t s, int b0, int n, const double* start, int period) {
  namespace rp = mpcq::replan;
  rp::MissionArgs a;
  a.traj = t.traj; a.Tmax = t.Tmax; a.lens = t.len; a.idx = t.idx; a.finished = t.finished;
  a.start = start; a.wp = ms.d_wp.p; a.legs = ms.d_legs.p;
  a.L = ms.L; a.n_wp = ms.n_wp; a.order = ms.order;
  a.dt = ms.dt;
  a.b0 = b0; a.n = n; a.period = period;
  const Mission::Ints d = ms.ints(B);
  a.leg = d.leg; a.installed = d.installed; a.last_code = d.last_code; a.claim = d.claim;
  a.leg_code = d.leg_code; a.leg_period = d.leg_period;
  a.info = ms.nonlinear ? ms.d_info.p : nullptr;
  const mpcq_nl::Opts o = ms.opts;
  if (ms.nonlinear)
    hipLaunchKernelGGL(rp::mission_kernel<rp::NlLds>, dim3(rp::mission_grid(n)), dim3(64), sizeof(rp::MissionLds<rp::NlLds>), s, a, o);
  else
    hipLaunchKernelGGL(rp::mission_kernel<rp::Lds>, dim3(rp::mission_grid(n)), dim3(64), sizeof(rp::MissionLds<rp::Lds>), s, a, o);
}

// ---- flight scoreboard (mpcq_score_*, mpcq_score.hpp): one row of 16 doubles per quadrotor and flight slot on the device, folded by a
// launch behind every period.
struct Score {
  bool on = false;
  int F = 0, tail_rows = 0;
  long long periods = 0;    // periods issued since mpcq_score_start / mpcq_score_clear
  DevBuf<double> d_table;   // [B,F,16]
  DevBuf<int> d_int;        // ints(B)
  // The layout of d_int: cur [B] | used [B] | overflow [B].  (mpcq::score::score_init_kernel takes the block as a whole and zeroes
  // 3 * B ints: the one other place that knows it.)
  struct Ints { int *cur, *used, *overflow; };
  static size_t n_ints(size_t B) { return 3 * B; }
  Ints ints(size_t B) const { return Ints{d_int.p, d_int.p + B, d_int.p + 2 * B}; }
};
// behind the recorder's row, in front of any plant launch: period `sper` of the scoreboard for the quadrotors [b0, b0 + n) of B
static void score_launch(const Score& sc, const EngineView& v, size_t B, hipStream_t s, int b0, int n, long long sper, const double* xmeas) {
  mpcq::score::Args a;
  const Score::Ints d = sc.ints(B);
  a.table = sc.d_table.p; a.cur = d.cur; a.used = d.used; a.overflow = d.overflow;
  a.F = sc.F; a.tail_rows = sc.tail_rows; a.b0 = b0; a.n = n; a.period = (double)sper;
  a.xmeas = xmeas; a.cost = v.cost; a.traj = v.traj;
  a.tlen = v.len; a.idx = v.idx; a.finished = v.finished; a.status = v.status; a.qp_iter = v.qp_iter;
  a.Tmax = v.Tmax; a.N = v.N; a.skip = v.skip;
  hipLaunchKernelGGL(mpcq::score::score_kernel, dim3(mpcq::score::grid((long)n * mpcq::score::W)), dim3(mpcq::score::BLOCK), 0, s, a);
}

// ---- exploration (mpcq_explore_*, mpcq_explore.hpp): the rules, the envelope of every quadrotor and the log of the limits it chose, on
// the device.  On only while a mission is: it writes into the mission's legs table (end_exploration).
struct Explore {
  bool on = false;
  DevBuf<mpcq_explore_rule> d_rules;   // [B]
  DevBuf<unsigned char> d_mask;        // [B,L]
  DevBuf<double> d_f64;                // f64(B)
  DevBuf<int64_t> d_samples;           // [B]
  // The layout of d_f64, and of the host image mpcq_explore_start fills (nl = B * L): env [B,3,2] | leg_limits [B,L,3]
  struct F64 { double *env, *leg_limits; };
  static size_t n_f64(size_t B, size_t nl) { return B * 6 + nl * 3; }
  static F64 f64_at(double* p, size_t B) { return F64{p, p + B * 6}; }
  F64 f64(size_t B) const { return f64_at(d_f64.p, B); }
};
// behind the score's launch, in front of the plant and mission launches: the period's sample into the envelopes of the quadrotors
// [b0, b0 + n) of B and the limits of the legs the mission launch of this period is about to plan (mpcq_explore.hpp)
static void explore_launch(const Explore& ex, const Mission& ms, const EngineView& v, size_t B, hipStream_t s, int b0, int n, const double* xmeas) {
  mpcq::explore::Args a;
  const Explore::F64 d = ex.f64(B);
  a.env = d.env; a.leg_limits = d.leg_limits; a.samples = ex.d_samples.p;
  a.rules = ex.d_rules.p; a.leg_mask = ex.d_mask.p;
  a.legs = ms.d_legs.p; a.leg = ms.ints(B).leg; a.L = ms.L;
  a.idx = v.idx; a.finished = v.finished; a.xmeas = xmeas;
  a.b0 = b0; a.n = n;
  hipLaunchKernelGGL(mpcq::explore::explore_kernel, dim3(mpcq::explore::grid(n)), dim3(mpcq::explore::BLOCK), 0, s, a);
}

// ---- the fleet (mpcq_fleet_*, mpcq_fleet.hpp): every quadrotor its own plant.  The table as the caller set it (what mpcq_fleet_get
// returns) and its field-major device form.
struct Fleet {
  bool on = false;
  long long period = 0;            // plant updates since period0 was set
  std::vector<mpcq_plant> plants;  // [B]
  DevBuf<double> d_tab;            // [fleet::NF][B]
};
// The fleet's plant update of the quadrotors [b0, b0 + n) of B, fleet period fper, in the place of the shared plant's launch
// (EngineT::plant_launch): n_sub substeps of sim_dt on xs [B,13] with the controls of the last step.
static void fleet_launch(const Fleet& fl, const EngineView& v, int B, hipStream_t s, int b0, int n, double* xs, int n_sub, double sim_dt, long long fper) {
  mpcq::fleet::Args a;
  a.tab = fl.d_tab.p; a.B = B; a.b0 = b0; a.n = n; a.g = v.g; a.period = (double)fper;
  a.xs = xs; a.w = v.w; a.n_sub = n_sub; a.sim_dt = sim_dt;
  hipLaunchKernelGGL(mpcq::fleet::fleet_plant_kernel, dim3((n + 63) / 64), dim3(64), 0, s, a);
}

// ---- the sensor (mpcq_sensor_*, mpcq_sensor.hpp): noise, bias, latency and dropout between plant and controller.  The table in its
// field-major device form, the ring of samples, the delivered measurement (what the step of mpcq_sim_steps solves from) and its age.
struct Sensor {
  bool on = false;
  int depth = 1, judge = MPCQ_SENSOR_JUDGE_MEASURED;
  long long period = 0, period0 = 0, index0 = 0;   // the next sensor period; the first; the global index of quadrotor 0
  uint64_t seed = 0;
  DevBuf<double> d_tab;      // [sensor::NF][B]
  DevBuf<long long> d_win;   // [sensor::NI][B]: out_from | out_to
  DevBuf<int> d_int;         // delay [B] | age [B]
  DevBuf<double> d_ring;     // the ring [depth][13][B] | the delivered measurement [B][13]: out(B)
  // The layout of d_ring and d_int as sensor_kernel knows them: the delivered measurement behind the ring, age behind delay
  double* out(size_t B) const { return d_ring.p + (size_t)depth * 13 * B; }
  int* age(size_t B) const { return d_int.p + B; }
};
// In front of everything else a control period issues: sensor period nper for the quadrotors [b0, b0 + n) of B, from the plant state
// v.plant into sn.out(B).  The measurement is float64 in both precisions: nothing here depends on the engine's.
static void sensor_launch(const Sensor& sn, const EngineView& v, int B, hipStream_t s, int b0, int n, long long nper) {
  mpcq::sensor::Args a;
  a.tab = sn.d_tab.p; a.win = sn.d_win.p; a.ints = sn.d_int.p; a.B = B; a.b0 = b0; a.n = n; a.depth = sn.depth;
  a.period = nper; a.since = nper - sn.period0; a.index0 = sn.index0;
  a.key0 = (unsigned)(sn.seed & 0xffffffffull); a.key1 = (unsigned)(sn.seed >> 32);
  a.x = v.plant; a.ring = sn.d_ring.p;
  hipLaunchKernelGGL(mpcq::sensor::sensor_kernel, dim3((n + 63) / 64), dim3(64), 0, s, a);
}

// ---- staging of the replan entry points (mpcq_replan, mpcq_replan_nonlinear, mpcq_replan_circle) and of mpcq_replace_trajectories
struct ReplanStaging {
  DevBuf<double> d_in;    // replan: the caller's part (waypoints [B,n_wp,3], or radius [B] | v_max [B]) | starts [B,3] | extra; replace: the rows
  DevBuf<int> d_int;      // ints(B)
  // The layout of d_int.  A replan: mask [B] | result codes [B].  mpcq_replace_trajectories: indices [B] | lengths [B], in the same places.
  struct Ints { int *mask, *code, *idx, *len; };
  static size_t n_ints(size_t B) { return 2 * B; }
  Ints ints(size_t B) const { return Ints{d_int.p, d_int.p + B, d_int.p, d_int.p + B}; }
};
// Quadrotors [b0, b0 + n) that advance by one launch per period: the stream their periods are issued on and, for a group of mpcq_sim_steps
// on a stream of its own, the event that marks the end of its part of a call.
struct Group {
  int b0, n;
  hipStream_t stream;
  hipEvent_t done;
};
// Stream, events and communicator of an engine.  A base class of mpcq_engine because bases are destroyed behind members: every device
// buffer the engine's members own is freed first, then the events, the streams and the communicator go, in this order.
struct EngineQueues {
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  std::vector<hipEvent_t> kev;   // per-launch event pairs of the last sim_steps call
  std::vector<Group> groups;     // [0, n_groups): the batch as mpcq_sim_steps runs it; [n_groups]: as one launch on `stream` (EngineT::init)
  hipEvent_t gstart = nullptr;   // more than one group: the other groups' streams start behind it
  void* comm = nullptr;
  bool comm_borrowed = false;   // comm belongs to another engine of this process (mpcq_comm_share)
  ~EngineQueues() {
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev1) (void)hipEventDestroy(ev1);
    for (hipEvent_t ev : kev) (void)hipEventDestroy(ev);
    for (const Group& g : groups) if (g.done) (void)hipEventDestroy(g.done);
    if (gstart) (void)hipEventDestroy(gstart);
    for (const Group& g : groups) if (g.stream != stream) (void)hipStreamDestroy(g.stream);
    if (stream) (void)hipStreamDestroy(stream);
    if (comm && !comm_borrowed && g_rccl.CommDestroy) g_rccl.CommDestroy(comm);
  }
};
struct mpcq_engine : EngineQueues {
  // (deleted with the engine's device current, mpcq_destroy: the destructors of the members free device memory, and a guard in a
  //  destructor's body would be gone before the first of them runs)
  virtual ~mpcq_engine() { for (void* p : arrays) (void)hipFree(p); }
  mpcq_config cfg;
  std::vector<double> basis, theta;
  int B = 0, N = 0, nb = 0, threads = 64;
  double last_time = 0;
  bool have_traj = false, timed = false;
  bool tuning_env = false;   // MPCQ_TUNING=1: measurement scripts may override tuning fields through the environment
  int nranks = 1;
  std::vector<void*> arrays;     // the device arrays of fixed size (EngineT::dalloc), freed with the engine
  double* d_stats5 = nullptr;
  int n_groups = 1;              // groups of mpcq_sim_steps (mpcq_tuning.groups; EngineT::init)
  double ktime = 0, kmin = 0, kmax = 0;   // HIP-event time of the timed step-kernel launches: total, fastest, slowest
  int klaunches = 0;
  bool have_sim = false;         // mpcq_sim_reset has set the plant state
  ReplanStaging rp;              // mpcq_replan* / mpcq_replace_trajectories
  Recorder rec;                  // mpcq_record_start .. mpcq_record_stop
  BlackBox bb;                   // mpcq_blackbox_start .. mpcq_blackbox_stop
  Mission ms;                    // mpcq_mission_set .. mpcq_mission_stop
  Score sc;                      // mpcq_score_start .. mpcq_score_stop
  Fleet fl;                      // mpcq_fleet_set .. mpcq_fleet_stop
  Explore ex;                    // mpcq_explore_start .. mpcq_explore_stop (or the end of the mission: end_exploration)
  Sensor sn;                     // mpcq_sensor_start .. mpcq_sensor_stop
  // The ticket of the period about to be issued, the one place the features' counters advance.  control: a control period (mpcq_step,
  // mpcq_step_device_async, every period of mpcq_sim_steps) -- the recorder, the black box, the mission and the score count it. plant: a plant update
  // (every period of mpcq_sim_steps, mpcq_sim_plant_period) -- the fleet period advances with it, never with a step alone.  sense: a
  // measurement through the sensor (every period of mpcq_sim_steps, mpcq_sensor_sample) -- never a step that takes the caller's.
  Tick next_tick(bool control, bool plant, bool sense = false) {
    Tick t;
    if (control) {
      t.row = rec.next_row();
      if (bb.on) { t.bper = bb.periods++; t.bslot = (int)(t.bper % bb.D); }
      if (ms.on) t.mper = (int)ms.periods++;
      if (sc.on) t.sper = sc.periods++;
    }
    if (plant && fl.on) t.fper = fl.period++;
    if (sense && sn.on) t.nper = sn.period++;
    return t;
  }
  // An exploration ends with the mission it explores for, or when that mission's queue is replaced: its launch writes limits into the
  // mission's legs table, which is gone then.
  void end_exploration() { ex = Explore(); }
  // RGP read-out (mpcq_rgp_predict / mpcq_record_predict, mpcq_predict.hpp): K_x^-1 as computed at create, in double, and device scratch
  std::vector<double> kxinv64;
  struct PredictScratch {
    DevBuf<double> Kinv, basis, xq, Jt, out;
    DevBuf<int> pos;
  } pr;
  // device trainer (mpcq_rgp_train / mpcq_record_train, mpcq_train.hpp): scratch sized by the request
  struct TrainScratch {
    DevBuf<double> in;      // caller samples: v_body [S,T,3] | a_drag [S,T,3]
    DevBuf<double> model;   // theta [3,3] | K_x [3,nb,nb] | a caller's model: basis [3,nb] | K_x^-1 [3,nb,nb]
    DevBuf<double> out;     // mu | C | mu_eta | C_eta | K_x^-1 of every regressor
    DevBuf<int> pos;
  } tr;
  virtual int rgp_predict(const double* xq, int M, int per_quad, double* mean, double* var) = 0;
  virtual EngineView view() = 0;
  virtual int init() = 0;
  virtual int reset() = 0;
  virtual int set_trajectories(const double*, const int32_t*, int32_t) = 0;
  virtual int set_reference(const double*, const double*) = 0;
  virtual int set_params(const double*) = 0;
  virtual int solve(const double*) = 0;
  virtual int get_x(int, double*) = 0;
  virtual int get_u(int, double*) = 0;
  virtual int get_cost(double*) = 0;
  virtual int get_int(int which, int32_t*) = 0;
  virtual int predict(const double*, const double*, double, double*) = 0;
  virtual int regress(const double*, const double*) = 0;
  virtual int get_rgp(double*, double*) = 0;
  virtual int step(const double*, double*, double*) = 0;
  virtual int step_device(const double*, double*) = 0;
  virtual int sim_reset(const double*) = 0;
  virtual int sim_steps(int, int, double) = 0;
  virtual int sim_run(int, int, double) = 0;
  virtual int sim_get(double*, double*) = 0;
  virtual int stats(double*) = 0;
  virtual int get_prof(unsigned long long*) = 0;
  virtual int get_order(int32_t*) = 0;
  virtual int get_command(double*, double*, double*) = 0;
  virtual int get_finished(int32_t*) = 0;
  virtual int get_chunk(double*) = 0;
  virtual int sim_plant(const double*, int, double) = 0;
  virtual int get_solver_state(int32_t*, double*, int32_t*) = 0;
  virtual int set_solver_state(const int32_t*, const double*, const int32_t*) = 0;
  virtual int get_state(double*, double*, double*, double*, double*, int32_t*, int32_t*) = 0;
  virtual int set_state(const double*, const double*, const double*, const double*, const double*, const int32_t*, const int32_t*) = 0;
};

namespace {

// ---- RGP read-out: the one evaluation routine behind mpcq_rgp_predict (live state, TQ = the engine's precision) and
// mpcq_record_predict (rows of the recorder's float64 buffers in place).  Set s reads mu / C at slab s (pos_host == nullptr) or at slab
// (row0 + k) * count + pos[j] with (j, k) = (s / nrows, s % nrows); outputs [nsets][3][M] go straight to the caller's arrays.
// the engine's own basis and K_x^-1 in double on the device (the step kernel's copies have the engine's precision): uploaded on first use
int rgp_model_on_device(mpcq_engine* e) {
  mpcq_engine::PredictScratch& pr = e->pr;
  const int nb = e->nb;
  if (pr.Kinv.p && pr.basis.p) return 0;
  HIP_TRY(pr.Kinv.grow((size_t)3 * nb * nb));
  HIP_TRY(pr.basis.grow((size_t)3 * nb));
  HIP_TRY(hipMemcpyAsync(pr.Kinv.p, e->kxinv64.data(), (size_t)3 * nb * nb * sizeof(double), hipMemcpyHostToDevice, e->stream));
  HIP_TRY(hipMemcpyAsync(pr.basis.p, e->basis.data(), (size_t)3 * nb * sizeof(double), hipMemcpyHostToDevice, e->stream));
  return 0;
}

template <typename TQ>
int predict_run(mpcq_engine* e, const TQ* mu, long mu_stride, const TQ* C, long C_stride, size_t nsets, const int* pos_host, int row0, int nrows, int count,
                const double* xq, int M, int per_quad, double* mean, double* var) {
  namespace pd = mpcq::predict;
  mpcq_engine::PredictScratch& pr = e->pr;
  const int nb = e->nb;
  hipStream_t s = e->stream;
  if (nsets * 3 > 0x7fffffffull) return fail(MPCQ_ERR_INVALID, "RGP read-out: too many (quadrotor, row) sets for one call");
  if (const int rc = rgp_model_on_device(e)) return rc;
  const size_t nq = (per_quad ? nsets : 1) * 3 * (size_t)M, no = nsets * 3 * (size_t)M;
  HIP_TRY(pr.xq.grow(nq));
  HIP_TRY(pr.out.grow(no * ((mean ? 1 : 0) + (var ? 1 : 0))));
  if (!per_quad) HIP_TRY(pr.Jt.grow((size_t)3 * (nb + 1) * M));
  HIP_TRY(hipMemcpyAsync(pr.xq.p, xq, nq * sizeof(double), hipMemcpyHostToDevice, s));
  if (pos_host) {
    HIP_TRY(pr.pos.grow((size_t)count));
    HIP_TRY(hipMemcpyAsync(pr.pos.p, pos_host, (size_t)count * sizeof(int), hipMemcpyHostToDevice, s));
  }
  pd::Args<TQ> a;
  std::memset(&a, 0, sizeof(a));
  a.mu = mu; a.C = var ? C : nullptr; a.mu_stride = mu_stride; a.C_stride = C_stride;
  a.pos = pos_host ? pr.pos.p : nullptr; a.row0 = row0; a.nrows = nrows; a.count = count;
  a.Kinv = pr.Kinv.p; a.basis = pr.basis.p;
  for (int d = 0; d < 3; ++d) {
    const double Lh = e->theta[3 * d], sf = e->theta[3 * d + 1];
    a.sf2[d] = sf * sf; a.hl2[d] = 0.5 / (Lh * Lh);
  }
  a.mean = mean ? pr.out.p : nullptr;
  a.var = var ? pr.out.p + (mean ? no : 0) : nullptr;
  a.nb = nb; a.M = M;
  if (per_quad) a.xq = pr.xq.p;
  else {   // J^T and b of the shared grid, once per call
    const double* d_xq = pr.xq.p;
    double *Jt = pr.Jt.p, *bq = Jt + (size_t)3 * nb * M;
    a.Jt = Jt; a.bq = bq;
    const size_t lds = (size_t)pd::layout(nb, false, true).total * sizeof(double);
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&pd::predict_prep_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(pd::predict_prep_kernel, dim3(3 * ((M + 63) / 64)), dim3(64), lds, s, d_xq, a.Kinv, a.basis,
                       a.sf2[0], a.sf2[1], a.sf2[2], a.hl2[0], a.hl2[1], a.hl2[2], nb, M, Jt, bq);
    HIP_TRY(hipGetLastError());
  }
  const bool stage = nb <= pd::STAGE_NB;
  const size_t lds = (size_t)pd::layout(nb, stage && a.C, per_quad != 0).total * sizeof(double);
  void (*k)(const pd::Args<TQ>) = stage ? &pd::predict_kernel<TQ, true> : &pd::predict_kernel<TQ, false>;
  HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(k, dim3((unsigned)(nsets * 3)), dim3(64), lds, s, a);
  HIP_TRY(hipGetLastError());
  if (mean) HIP_TRY(hipMemcpyAsync(mean, a.mean, no * sizeof(double), hipMemcpyDeviceToHost, s));
  if (var) HIP_TRY(hipMemcpyAsync(var, a.var, no * sizeof(double), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return 0;
}

// the check in front of everything that reads the trajectory slots (`who`: the entry point's name)
int needs_trajectories(mpcq_engine* e, const std::string& who) {
  if (e->have_traj && e->view().traj) return 0;
  return fail(MPCQ_ERR_STATE, who + " needs mpcq_set_trajectories first");
}
// the recorder's read-back: rows [rows][count][W] on the device -> out [count][rows][W] in the caller's order
template <typename V> int rec_read(mpcq_engine* e, const V* src, int W, V* out) {
  const Recorder& r = e->rec;
  const size_t n = (size_t)r.rows * r.count * W;
  if (!n) return 0;
  std::vector<V> tmp(n);
  HIP_TRY(hipMemcpyAsync(tmp.data(), src, n * sizeof(V), hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  for (int j = 0; j < r.count; ++j)
    for (int k = 0; k < r.rows; ++k)
      std::memcpy(out + ((size_t)j * r.rows + k) * W, tmp.data() + ((size_t)k * r.count + r.pos[j]) * W, W * sizeof(V));
  return 0;
}
// ---- incident recorder: what the mpcq_blackbox_* entry points share
// What a quadrotor's ring holds now, from its device state: its first period p0, the number of rows and the row of the firing period
struct BoxRows { long long p0; int rows, fired_row; };
BoxRows box_rows(const BlackBox& r, int state, long long fired, long long first) {
  if (fired < 0) {   // armed: the last D periods since `first`
    const long long rows = std::max(0LL, std::min((long long)r.D, r.periods - first));
    return BoxRows{r.periods - rows, (int)rows, -1};
  }
  // fired: the incident, from `pre` periods in front of it (older rows the ring still holds are on their way out: the rows behind the
  // firing period overwrite them) to the last period written
  const long long last = state == mpcq::blackbox::FROZEN ? fired + r.post : r.periods - 1;
  const long long p0 = std::max(first, fired - r.pre);
  return BoxRows{p0, (int)(last - p0 + 1), (int)(fired - p0)};
}
// The device state of the selection, behind everything the engine has enqueued (sorted order)
struct BoxState { std::vector<int> ints; std::vector<long long> i64; };
int box_state(mpcq_engine* e, BoxState& h) {
  const BlackBox& r = e->bb;
  h.ints.resize(3 * (size_t)r.count); h.i64.resize(2 * (size_t)r.count);
  HIP_TRY(hipMemcpyAsync(h.ints.data(), r.d_int.p, h.ints.size() * sizeof(int), hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipMemcpyAsync(h.i64.data(), r.d_i64.p, h.i64.size() * sizeof(long long), hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  return 0;
}
// The checks of a read-out's subset (`who`: the entry point): which [n] positions in the caller's selection, or NULL for all of it.
// sel: the places in the sorted selection, in the caller's order.
int box_subset(const std::string& who, const BlackBox& r, const int32_t* which, int32_t n, std::vector<int>& sel) {
  if (which && n < 0) return fail(MPCQ_ERR_INVALID, who + ": n must be >= 0");
  const int m = which ? n : r.count;
  sel.resize(m);
  std::vector<char> seen(r.count, 0);
  for (int i = 0; i < m; ++i) {
    const int j = which ? which[i] : i;
    if (j < 0 || j >= r.count) return fail(MPCQ_ERR_INVALID, who + ": position " + std::to_string(j) + " outside the selection [0, " + std::to_string(r.count) + ")");
    if (seen[j]++) return fail(MPCQ_ERR_INVALID, who + ": duplicate position " + std::to_string(j));
    sel[i] = r.pos[j];
  }
  return 0;
}
// One field's rings of the subset in time order: src [D][count][W] on the device -> out [n][D][W] on the host, through the staging block
template <typename V> int box_read(mpcq_engine* e, const std::string& who, const V* src, int W, V fill, const int32_t* which, int32_t n, V* out) {
  namespace bx = mpcq::blackbox;
  BlackBox& r = e->bb;
  std::vector<int> sel;
  if (const int rc = box_subset(who, r, which, n, sel)) return rc;
  const size_t m = sel.size(), total = m * r.D * W;
  if (!total) return 0;
  if (!out) return fail(MPCQ_ERR_INVALID, "null argument");
  if ((total + 63) / 64 > 0x7fffffffull) return fail(MPCQ_ERR_INVALID, who + ": too many values for one call (n x D x width): read a subset");
  BoxState h;
  if (const int rc = box_state(e, h)) return rc;
  std::vector<int> meta(2 * m);   // which | rows
  std::vector<long long> p0(m);
  for (size_t i = 0; i < m; ++i) {
    const int j = sel[i];
    const BoxRows br = box_rows(r, h.ints[j], h.i64[j], h.i64[r.count + j]);
    meta[i] = j; meta[m + i] = br.rows; p0[i] = br.p0;
  }
  const bool ints = sizeof(V) == sizeof(int);
  const std::string no_mem = who + ": cannot allocate the staging block of " + std::to_string(total * sizeof(V)) + " bytes";
  int rc;
  if ((rc = grow_or_fail(r.d_stage_int, 2 * m + (ints ? total : 0), no_mem)) || (rc = grow_or_fail(r.d_stage_p0, m, no_mem))) return rc;
  if (!ints && (rc = grow_or_fail(r.d_stage, total, no_mem))) return rc;
  V* d_out = ints ? (V*)(r.d_stage_int.p + 2 * m) : (V*)r.d_stage.p;
  HIP_TRY(hipMemcpyAsync(r.d_stage_int.p, meta.data(), meta.size() * sizeof(int), hipMemcpyHostToDevice, e->stream));
  HIP_TRY(hipMemcpyAsync(r.d_stage_p0.p, p0.data(), m * sizeof(long long), hipMemcpyHostToDevice, e->stream));
  const int *d_which = r.d_stage_int.p, *d_rows = r.d_stage_int.p + m;
  const long long* d_p0 = r.d_stage_p0.p;
  const int D = r.D, count = r.count;
  hipStream_t s = e->stream;
  hipLaunchKernelGGL(bx::gather_kernel<V>, dim3((unsigned)((total + 63) / 64)), dim3(64), 0, s, src, d_which, d_p0, d_rows, (long)total, D, W, count, fill, d_out);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(out, d_out, total * sizeof(V), hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  return 0;
}
// The state of the selected places (d_mask [count] in sorted order on the device, or nullptr: all) to armed, the ring beginning with `first`
int box_init(mpcq_engine* e, const int* d_mask, long long first) {
  const mpcq::blackbox::State st = e->bb.state();
  const int count = e->bb.count;
  hipStream_t s = e->stream;
  hipLaunchKernelGGL(mpcq::blackbox::init_kernel, dim3((count + 63) / 64), dim3(64), 0, s, st, d_mask, count, first);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(e->stream));
  return 0;
}
// What the seven *_stop entry points do with their feature f of e (not_on: the error of a feature that is not on)
template <typename F> int feature_stop(mpcq_engine* e, F& f, const char* not_on) {
  if (!f.on) return fail(MPCQ_ERR_STATE, not_on);
  HIP_TRY(hipStreamSynchronize(e->stream));   // (launches of an mpcq_step_device_async may still use the feature's buffers)
  f = F();
  return 0;
}

template <typename T>
struct EngineT : mpcq_engine {
  mpcq::DevModel<T> m;
  mpcq::DevState<T> st;
  mpcq::Lds L;
  size_t lds_bytes = 0;
  int resident_per_cu = 0;   // workgroups of the lockstep instance one CU holds at once (LDS and registers)
  void (*kstep)(const mpcq::DevModel<T>, const mpcq::DevState<T>, const int) = nullptr;
  void (*krun)(const mpcq::DevModel<T>, const mpcq::DevState<T>, const int) = nullptr;   // free-running variant (mpcq_sim_run)
  T *d_basis = nullptr, *d_Kxinv = nullptr, *d_Kx = nullptr;
  double* h_pin = nullptr;   // pinned staging of the host-buffer step: [x_meas B*13 | w B*4 | x_pred B*13]
  double *d_xin = nullptr, *d_uin = nullptr, *d_tmp = nullptr, *d_xs = nullptr, *d_vb = nullptr, *d_ad = nullptr;
  DevBuf<double> d_traj;     // [B][Tmax][13] (mpcq_set_trajectories)
  int* d_tlen = nullptr;
  int* d_order = nullptr;    // launch order of the lockstep periods (order_kernel); used when the batch exceeds what the device holds at once
  bool use_order = false;
  bool split_plant = false;   // the plant update between two lockstep periods as its own launch (streaming batches), see sim_steps
  DevBuf<double> d_cmd;      // [B*8] rotor thrusts, collective thrust, body rates (mpcq_get_command); also the chunk read-back
  std::vector<T> hbuf;
  std::vector<double> Kx;

  ~EngineT() override { if (h_pin) (void)hipHostFree(h_pin); }

  EngineView view() override {
    return EngineView{d_traj.p, d_tlen, st.idx, st.finished, d_xs, m.Tmax, st.cost, st.status, st.qp_iter, st.w, N, m.skip, (double)m.g};
  }
  // a zero-filled device array of n elements (at least one: nb = 0) that lives as long as the engine
  template <typename P> int dalloc(P*& p, size_t n) {
    HIP_TRY(hipMalloc((void**)&p, (n ? n : 1) * sizeof(*p)));
    arrays.push_back(p);
    HIP_TRY(hipMemsetAsync(p, 0, (n ? n : 1) * sizeof(*p), stream));
    return 0;
  }
  // a copy on the engine's stream, complete when the call returns
  int copy_sync(void* dst, const void* src, size_t bytes, hipMemcpyKind kind) {
    HIP_TRY(hipMemcpyAsync(dst, src, bytes, kind, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return 0;
  }
  int h2q(T* dst, const double* src, size_t n) {
    hbuf.resize(n);
    for (size_t i = 0; i < n; ++i) hbuf[i] = (T)src[i];
    return copy_sync(dst, hbuf.data(), n * sizeof(T), hipMemcpyHostToDevice);
  }
  int h2d(double* dst, const double* src, size_t n) { return copy_sync(dst, src, n * sizeof(double), hipMemcpyHostToDevice); }
  int d2h(double* dst, const double* src, size_t n) { return copy_sync(dst, src, n * sizeof(double), hipMemcpyDeviceToHost); }
  int q2h(double* dst, const T* src, size_t n) {
    hbuf.resize(n);
    if (const int rc = copy_sync(hbuf.data(), src, n * sizeof(T), hipMemcpyDeviceToHost)) return rc;
    for (size_t i = 0; i < n; ++i) dst[i] = (double)hbuf[i];
    return 0;
  }

  int init() override {
    const mpcq_config& c = cfg;
    HIP_TRY(hipSetDevice(c.device));
    HIP_TRY(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    HIP_TRY(hipEventCreate(&ev0));
    HIP_TRY(hipEventCreate(&ev1));
    std::memset(&m, 0, sizeof(m));
    std::memset(&st, 0, sizeof(st));
    m.N = N; m.nb = nb; m.skip = c.skip; m.Tmax = 0; m.B = B;
    const bool f32 = sizeof(T) == 4;
    m.qp_max_iter = c.qp_max_iter > 0 ? c.qp_max_iter : 60;
    // (float: the interior point is not asked for more than 1e-5 -- below that its complementarity collapses while the float residual
    //  stalls, and a stage Hessian loses definiteness or the iterate its finiteness; the answer's accuracy comes from the refinement
    //  against fp64 residuals behind it, not from the interior point's own tolerance.  Smaller values are raised to 1e-5.)
    m.qp_tol = (T)(c.qp_tol > 0 ? c.qp_tol : (f32 ? 1e-5 : 1e-11));
    if (f32 && m.qp_tol < (T)1e-5) m.qp_tol = (T)1e-5;
    m.eps = f32 ? (T)6e-8 : (T)1.1e-16;
    // ---- solver tuning: mpcq_config.tune (0 = default), validated by mpcq_create_sized; with MPCQ_TUNING=1 the environment
    // overrides a field (measurement scripts).  How the defaults were measured: DESIGN.md section 3.3.
    const mpcq_tuning& tu = c.tune;
    const bool env = tuning_env = getenv("MPCQ_TUNING") && atoi(getenv("MPCQ_TUNING")) != 0;
    if (!env) {   // advisor finding: a measurement script that forgets MPCQ_TUNING=1 would otherwise compare identical configurations
      static const char* const knobs[] = {"MPCQ_WARM_MAX", "MPCQ_WARM_RETRY", "MPCQ_FLIP_MAX", "MPCQ_ABORT_PINS", "MPCQ_ABORT_WRONG", "MPCQ_POLISH_MAX", "MPCQ_PIN_RATIO",
                                          "MPCQ_IPM_MU0", "MPCQ_IPM_MARGIN", "MPCQ_IPM_TOL", "MPCQ_STAGE_MEM", "MPCQ_GENERIC", "MPCQ_BLOCK_ORDER", "MPCQ_KEV_STRIDE", "MPCQ_SPLIT_PLANT", "MPCQ_GROUPS"};
      static bool warned = false;
      for (const char* k : knobs)
        if (!warned && getenv(k)) { fprintf(stderr, "mpcq: %s is set but MPCQ_TUNING=1 is not: the environment is ignored (use mpcq_config.tune)\n", k); warned = true; }
    }
    auto ienv = [&](const char* name, int v) { const char* t = env ? getenv(name) : nullptr; return t ? atoi(t) : v; };
    auto fenv = [&](const char* name, double v) { const char* t = env ? getenv(name) : nullptr; return t ? atof(t) : v; };
    auto off = [](int v) { return v < 0 ? 0 : v; };   // -1 = "never": the kernel's encoding is 0 (flip_max: -1)
    // (float: 1e-5.  The mixed-precision method judges multipliers on double residuals, so a hand-over as tight as fp64's pays -- bench
    //  workload, 200 lockstep periods: 1e-4 / pin_ratio 1 2.70 M steps/s, 1e-5 / 0.2 2.89 M, 1e-6 / 0.2 2.94 M -- but below 1e-5 the float
    //  interior point itself loses a stage Hessian's definiteness now and then at N = 50 (the active-set method then takes over from its
    //  last iterate, solve_qp): 1e-5 keeps it out of that regime)
    m.ipm_tol = (T)fenv("MPCQ_IPM_TOL", tu.ipm_tol > 0 ? tu.ipm_tol : (f32 ? 1e-5 : 1e-6));
    // fp64 passes alternate between a multiplier check and an affine solve: twice the count of fp32's
    m.polish_max = ienv("MPCQ_POLISH_MAX", tu.polish_max ? off(tu.polish_max) : (f32 ? 12 : 16));
    // passes of the warm active-set attempt before falling back to the interior point (fp64: one factorisation each, an
    // interior-point solve costs about 15 of them)
    // 12 passes in both precisions since the factorisation stage of a pass costs little more than an interior-point one (round 4: 534 -> ~330
    // instructions): 6 -> 12 is + 3-6 % on the bench workload (four seeds), + 23 % on the round-1 spline flights 150 periods in; 16 / 24 add nothing
    m.warm_max = ienv("MPCQ_WARM_MAX", tu.warm_max > 0 ? tu.warm_max : 12);
    m.warm_retry = ienv("MPCQ_WARM_RETRY", tu.warm_retry > 0 ? tu.warm_retry : 1);
    m.ipm_margin = (T)fenv("MPCQ_IPM_MARGIN", tu.ipm_margin > 0 ? tu.ipm_margin : 0.1);
    // hand-over from the interior point: an input joins the working set when its multiplier exceeds pin_ratio x its slack
    // (weakly active ones are pinned at once, wrongly pinned ones leave through the multiplier check of the same pass)
    m.pin_ratio = (T)fenv("MPCQ_PIN_RATIO", tu.pin_ratio > 0 ? tu.pin_ratio : 0.2);
    // complementarity of the interior start in units of the gradient scale: the start is the previous solution pushed inside
    // the box, i.e. close to the new optimum, a small value makes it a warm start
    m.ipm_mu0 = (T)fenv("MPCQ_IPM_MU0", tu.ipm_mu0 > 0 ? tu.ipm_mu0 : 1e-4);
    // a fallback solve whose solution changed more than this many bound states against the previous one marks a quadrotor whose
    // saturated inputs flip between rotors every period: its next solve goes to the interior point directly
    m.flip_max = ienv("MPCQ_FLIP_MAX", tu.flip_max ? tu.flip_max : 2);
    // early exits of the warm attempt: a first pass that pins >= abort_pins inputs, a multiplier check with >= abort_wrong
    // wrong signs (the most aggressive pair that costs the round-1 spline flights nothing)
    m.abort_pins = ienv("MPCQ_ABORT_PINS", tu.abort_pins ? off(tu.abort_pins) : (N > 20 ? N / 2 : 10));
    m.abort_wrong = ienv("MPCQ_ABORT_WRONG", tu.abort_wrong ? off(tu.abort_wrong) : (N > 20 ? (9 * N) / 20 : 9));
    if (m.ipm_tol < m.qp_tol) m.ipm_tol = m.qp_tol;
    m.h = c.T / c.N; m.dt_pred = c.dt_pred;
    m.finish_r = c.finish_radius > 0 ? c.finish_radius : 1.0;
    m.mass = c.mass; m.tmax = c.max_thrust; m.g = c.g; m.aero_drag = c.aero_drag;
    for (int i = 0; i < 3; ++i) { m.J[i] = c.J[i]; m.iJ[i] = 1.0 / c.J[i]; m.rotor_drag[i] = c.rotor_drag[i]; }
    m.imass = 1.0 / c.mass;
    for (int i = 0; i < 4; ++i) {
      m.xf[i] = c.x_f[i]; m.yf[i] = c.y_f[i]; m.zl[i] = c.z_l_tau[i];
      m.ulb[i] = c.u_lb[i]; m.uub[i] = c.u_ub[i]; m.uref[i] = c.u_ref[i];
    }
    for (int i = 0; i < 17; ++i) m.W[i] = c.W[i];
    for (int i = 0; i < 13; ++i) m.We[i] = c.W_e[i];
    // RGP constants: K_x = K(X,X) + sn^2 I and its inverse (RGP.__init__, src/gp/RGP.py:140-157)
    Kx.assign((size_t)3 * nb * nb, 0.0);
    std::vector<double> Kxinv((size_t)3 * nb * nb, 0.0);
    for (int d = 0; d < 3 && nb; ++d) {
      const double Lh = theta[3 * d], sf = theta[3 * d + 1], sn = theta[3 * d + 2];
      if (!(Lh > 0)) return fail(MPCQ_ERR_INVALID, "theta: length scale must be > 0");
      m.L2inv[d] = (T)(1.0 / (Lh * Lh)); m.sf2[d] = (T)(sf * sf); m.sn2[d] = (T)(sn * sn);
      std::vector<double> K, Ki;
      if (!rgp_axis_constants(basis.data() + (size_t)d * nb, nb, Lh, sf, sn, K, Ki)) return fail(MPCQ_ERR_INVALID, "K_x is not positive definite");
      std::copy(K.begin(), K.end(), Kx.begin() + (size_t)d * nb * nb);
      std::copy(Ki.begin(), Ki.end(), Kxinv.begin() + (size_t)d * nb * nb);
    }
    int rc;
    if ((rc = dalloc(d_basis, 3 * nb))) return rc;
    if ((rc = dalloc(d_Kxinv, (size_t)3 * nb * nb))) return rc;
    if ((rc = dalloc(d_Kx, (size_t)3 * nb * nb))) return rc;
    if (nb) {
      if ((rc = h2q(d_basis, basis.data(), 3 * nb))) return rc;
      if ((rc = h2q(d_Kxinv, Kxinv.data(), (size_t)3 * nb * nb))) return rc;
      if ((rc = h2q(d_Kx, Kx.data(), (size_t)3 * nb * nb))) return rc;
    }
    m.basis = d_basis; m.Kxinv = d_Kxinv;
    kxinv64 = Kxinv;   // (the device copy above is T-typed; mpcq_rgp_predict evaluates in double)
    const size_t Bz = B;
    if ((rc = dalloc(st.X, Bz * (N + 1) * 13))) return rc;
    if ((rc = dalloc(st.U, Bz * N * 4))) return rc;
    if ((rc = dalloc(st.mu, Bz * 3 * nb))) return rc;
    if ((rc = dalloc(st.C, Bz * 3 * nb * nb))) return rc;
    if ((rc = dalloc(st.xpp, Bz * 13))) return rc;
    if ((rc = dalloc(st.yref, Bz * N * 17))) return rc;
    if ((rc = dalloc(st.yrefN, Bz * 13))) return rc;
    if ((rc = dalloc(st.w, Bz * 4))) return rc;
    if ((rc = dalloc(st.xpred, Bz * 13))) return rc;
    if ((rc = dalloc(st.cost, Bz))) return rc;
    if ((rc = dalloc(st.stats, Bz * 4))) return rc;
    if ((rc = dalloc(st.has_prev, Bz))) return rc;
    if ((rc = dalloc(st.idx, Bz))) return rc;
    if ((rc = dalloc(st.status, Bz))) return rc;
    if ((rc = dalloc(st.qp_iter, Bz))) return rc;
    if ((rc = dalloc(st.qp_work, Bz))) return rc;
    if ((rc = dalloc(st.finished, Bz))) return rc;
    if ((rc = dalloc(d_tlen, Bz))) return rc;
    if ((rc = dalloc(d_xin, Bz * 13))) return rc;
    if ((rc = dalloc(d_uin, Bz * 4))) return rc;
    if ((rc = dalloc(d_tmp, Bz * 13))) return rc;
    if ((rc = dalloc(d_xs, Bz * 13))) return rc;
    if ((rc = dalloc(d_vb, Bz * 3))) return rc;
    if ((rc = dalloc(d_ad, Bz * 3))) return rc;
    if ((rc = dalloc(d_stats5, 8))) return rc;
#if defined(MPCQ_PROFILE) || defined(MPCQ_TRACE_NAN)
    if ((rc = dalloc(st.prof, Bz * mpcq::PF_N))) return rc;
#endif
#ifdef MPCQ_CHECKED
    if ((rc = dalloc(st.chk, 16))) return rc;
#endif
#ifdef MPCQ_DUMP_AT
    if ((rc = dalloc(m.dbg, Bz * 4096))) return rc;
#endif
    st.tlen = d_tlen; st.traj = nullptr; st.x_meas = d_xin;
    // Layout of the working set (mpcq::lds_layout): 0 everything in LDS | 1 the per-stage records (AB'', c, qv) in the per-instance
    // global record (L2 / MALL) | 2 "compact": the Riccati gains there as well, instances limited to 256 registers -- a second wave
    // per SIMD.  Rule: LDS when the whole batch is resident at once that way, otherwise the layout that holds more instances per CU,
    // the compact one only for batches beyond what layout 0 / 1 hold at once.  mpcq_config.tune.stage_mem overrides.
    int n_cu = 256;
    { hipDeviceProp_t prop; if (hipGetDeviceProperties(&prop, c.device) == hipSuccess && prop.multiProcessorCount > 0) n_cu = prop.multiProcessorCount; }
    const bool generic = ienv("MPCQ_GENERIC", tu.generic_kernel) != 0;
    mpcq::Lds Ls[3];
    size_t bytes[3], occ[3];
    mpcq::StepFn<T> ks[3], kr[3];
    ks[0] = &mpcq::step_kernel<mpcq::Cfg<T, false>>; ks[1] = &mpcq::step_kernel<mpcq::Cfg<T, true>>; ks[2] = &mpcq::step_kernel<mpcq::Cfg<T, true, 0, -1, false, true>>;
    // free-running launches (mpcq_sim_run): the any-shape instance, replaced below by a shape-specialised one where mpcq_spec.hip has it
    kr[0] = &mpcq::step_kernel<mpcq::Cfg<T, false, 0, -1, true>>; kr[1] = &mpcq::step_kernel<mpcq::Cfg<T, true, 0, -1, true>>;
    kr[2] = &mpcq::step_kernel<mpcq::Cfg<T, true, 0, -1, true, true>>;
    for (int l = 0; l < 3; ++l) {
      Ls[l] = mpcq::lds_layout(N, nb, l, sizeof(T) == 4);
      bytes[l] = mpcq::lds_bytes<T>(Ls[l]);
      // lockstep launches: shape-specialised instances (compile-time N and nb), from mpcq_spec.hip
      if (!generic)
        if (auto k = spec_step(N, nb, l, (T*)nullptr)) ks[l] = k;
      occ[l] = 0;
      if (bytes[l] <= 160 * 1024) {   // resident workgroups per CU: LDS and registers of the instance that would run
        int nblk = 0;
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(ks[l]), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes[l]));
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nblk, reinterpret_cast<const void*>(ks[l]), 64, bytes[l]) == hipSuccess && nblk > 0) occ[l] = (size_t)nblk;
        else occ[l] = (160 * 1024) / bytes[l];
      }
    }
    int layout = (occ[0] == 0 || (occ[1] > occ[0] && (size_t)B > occ[0] * n_cu)) ? 1 : 0;
    // (the compact instance is a few per cent slower per wave -- 256 registers, gains through L2 -- and adds memory-side traffic, so it
    //  takes a long stream of workgroups to pay.  Measured at N = 20, nb = 10, M steps/s layout 1 / compact: B = 2 048 5.03 / 4.83, 3 072
    //  7.04 / 6.68, 4 096 8.61 / 8.22, 6 144 9.91 / 10.49, 8 192 10.5 / 11.7, 16 384 9.5 / 10.6: from five rounds of layout 1 on.
    //  N = 50, nb = 50 (one against two per CU): B = 4 096 0.70 / 1.22.)
    {
      const size_t r1 = occ[layout] * n_cu;
      if (occ[2] > occ[layout] && (size_t)B >= 5 * r1) layout = 2;
    }
    if (tu.stage_mem) layout = tu.stage_mem - 1;
    if (const char* t = env ? getenv("MPCQ_STAGE_MEM") : nullptr) layout = (t[0] == 'c' || t[0] == 'C') ? 2 : ((t[0] == 'g' || t[0] == 'G') ? 1 : 0);
    if (occ[layout] == 0)
      return fail(MPCQ_ERR_INVALID, layout == 0 ? "per-instance working set exceeds 160 KiB LDS with the stage records in LDS (tune.stage_mem = 1)"
                                                : "per-instance working set exceeds 160 KiB LDS (N/nb too large for this precision)");
    m.gab = layout;
    if (env && getenv("MPCQ_VERBOSE"))
      fprintf(stderr, "mpcq: layout %d (%s), LDS %zu B per instance, %zu instances per CU; layouts 0/1/2: %zu/%zu/%zu B, %zu/%zu/%zu per CU\n", layout,
              layout == 0 ? "all LDS" : (layout == 1 ? "stage records in global memory" : "compact: stage records and gains in global memory"), bytes[layout], occ[layout],
              bytes[0], bytes[1], bytes[2], occ[0], occ[1], occ[2]);
    L = Ls[layout];
    lds_bytes = bytes[layout];
    resident_per_cu = (int)occ[layout];
    if ((rc = dalloc(st.stage, Bz * L.gtotal))) return rc;   // stage records (global placement) + multiplier rows + cost-to-go tiles (+ gains)
    // Launch order of a lockstep period: a batch beyond what the device holds at once is a stream of workgroups that ends with
    // its last one, so the quadrotors predicted to be expensive go first (mpcq::order_kernel in front of every step launch).
    // A batch that is resident as a whole starts all at once: no order needed.  tune.block_order: 1 = never, 2 = always.
    {
      const size_t resident = occ[layout] * (size_t)n_cu;
      const int bo = ienv("MPCQ_BLOCK_ORDER", tu.block_order);
      use_order = bo == 2 || (bo == 0 && (size_t)B > resident);
      if (use_order) {   // the identity until the first lockstep launch has computed an order (mpcq_get_block_order before that)
        if ((rc = dalloc(d_order, Bz))) return rc;
        std::vector<int> ident(Bz);
        for (size_t b = 0; b < Bz; ++b) ident[b] = (int)b;
        HIP_TRY(hipMemcpyAsync(d_order, ident.data(), Bz * sizeof(int), hipMemcpyHostToDevice, stream));
        HIP_TRY(hipStreamSynchronize(stream));
      }
      // The same distinction decides where the plant update of the on-device closed loop runs (sim_steps): at the head of the next
      // step launch (one launch per period; its RK4 substeps run on one lane of every workgroup: 6 k of a quadrotor's 172 k cycles)
      // or as its own launch of one THREAD per quadrotor.  A resident batch waits for its slowest quadrotor, which the 2.5 us at
      // the head hardly move, and saves a launch; a streaming batch pays those cycles in throughput.
      split_plant = ienv("MPCQ_SPLIT_PLANT", (size_t)B > resident ? 1 : 0) != 0;
      // Groups of mpcq_sim_steps (tune.groups; 0 = automatic).  A streaming batch ends every launch with a tail in which the device
      // drains (the last workgroups finish one by one: 13 % of the resident-wave slots of a B = 8 192 launch stand empty,
      // profiles/r6_pmc_icache_b8192.json) and the next period's launch cannot start before it has: cut into groups whose launches go to
      // streams of their own, the tail of one group's period is filled by the other groups' launches.  Every group advances in lockstep,
      // quadrotors are independent, a call still ends with every quadrotor K periods on: results do not depend on the grouping.
      // A resident batch has no tail to fill (what its launch waits for is its slowest quadrotor): one group unless asked otherwise.
      n_groups = ienv("MPCQ_GROUPS", tu.groups > 0 ? tu.groups : ((size_t)B > resident ? MPCQ_AUTO_GROUPS : 1));
      if (n_groups < 1) n_groups = 1;
      while (n_groups > 1 && B / n_groups < 8) n_groups -= 1;    // (a group holds at least one quadrotor of every launch-order class)
      const int per = ((B + n_groups - 1) / n_groups + 7) / 8 * 8;   // quadrotors per group (the last one takes what is left)
      for (int g = 0; g < n_groups; ++g) {   // (group 0 runs on the engine's own stream: one hardware queue less)
        const int b0 = std::min(B, g * per);
        groups.push_back(Group{b0, std::min(B, b0 + per) - b0, stream, nullptr});
        if (g == 0) continue;
        HIP_TRY(hipStreamCreateWithFlags(&groups[g].stream, hipStreamNonBlocking));
        HIP_TRY(hipEventCreateWithFlags(&groups[g].done, hipEventDisableTiming));
      }
      if (n_groups > 1) HIP_TRY(hipEventCreateWithFlags(&gstart, hipEventDisableTiming));
      groups.push_back(Group{0, B, stream, nullptr});   // mpcq_solve, mpcq_step, mpcq_step_device_async: always one launch over the batch
    }
    kstep = ks[layout];
    krun = kr[layout];
#ifdef MPCQ_SPEC_RUN_SHAPES
    if (!generic)
      if (auto k = spec_run(N, nb, layout, (T*)nullptr)) krun = k;
#endif
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(krun), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(kstep), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&mpcq::regress_kernel<T>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
    return reset();
  }

  int reset() override {
    const size_t Bz = B;
    HIP_TRY(hipMemsetAsync(st.X, 0, Bz * (N + 1) * 13 * sizeof(double), stream));
    HIP_TRY(hipMemsetAsync(st.U, 0, Bz * N * 4 * sizeof(double), stream));
    if (nb) HIP_TRY(hipMemsetAsync(st.mu, 0, Bz * 3 * nb * sizeof(T), stream));
    HIP_TRY(hipMemsetAsync(st.xpp, 0, Bz * 13 * sizeof(double), stream));
    HIP_TRY(hipMemsetAsync(st.stats, 0, Bz * 4 * sizeof(double), stream));
    HIP_TRY(hipMemsetAsync(st.has_prev, 0, Bz * sizeof(int), stream));
    HIP_TRY(hipMemsetAsync(st.idx, 0, Bz * sizeof(int), stream));
    HIP_TRY(hipMemsetAsync(st.status, 0, Bz * sizeof(int), stream));
    HIP_TRY(hipMemsetAsync(st.qp_iter, 0, Bz * sizeof(int), stream));
    HIP_TRY(hipMemsetAsync(st.finished, 0, Bz * sizeof(int), stream));
    std::vector<T> h((size_t)B * 3 * nb * nb);   // (read by the copy below: lives until the synchronise)
    if (nb) {  // C_0 = K_x for every instance and axis
      for (size_t b = 0; b < Bz; ++b)
        for (size_t i = 0; i < (size_t)3 * nb * nb; ++i) h[b * 3 * nb * nb + i] = (T)Kx[i];
      HIP_TRY(hipMemcpyAsync(st.C, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice, stream));
    }
    HIP_TRY(hipStreamSynchronize(stream));
    return 0;
  }

  int set_trajectories(const double* traj, const int32_t* len, int32_t Tmax) override {
    if (Tmax <= 0) return fail(MPCQ_ERR_INVALID, "Tmax must be positive");
    for (int b = 0; b < B; ++b)
      if (len[b] <= 0 || len[b] > Tmax) return fail(MPCQ_ERR_INVALID, "trajectory length out of range");
    HIP_TRY(d_traj.grow((size_t)B * Tmax * 13));
    m.Tmax = Tmax;
    int rc;
    if ((rc = h2d(d_traj.p, traj, (size_t)B * Tmax * 13))) return rc;
    HIP_TRY(hipMemcpyAsync(d_tlen, len, (size_t)B * sizeof(int), hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemsetAsync(st.idx, 0, (size_t)B * sizeof(int), stream));
    HIP_TRY(hipMemsetAsync(st.finished, 0, (size_t)B * sizeof(int), stream));
    HIP_TRY(hipStreamSynchronize(stream));
    st.traj = d_traj.p;
    have_traj = true;
    return 0;
  }
  int set_reference(const double* yref, const double* yrefN) override {
    int rc;
    if ((rc = h2d(st.yref, yref, (size_t)B * N * 17))) return rc;
    return h2d(st.yrefN, yrefN, (size_t)B * 13);
  }
  int set_params(const double* mu) override { return nb ? h2q(st.mu, mu, (size_t)B * 3 * nb) : 0; }

  // Checked build: every call that launched the step / regress kernel ends here -- the first out-of-range index or partial EXEC
  // mask the device code recorded turns the call into an error that names it (region tag, index, valid range, lane, workgroup,
  // program counter relative to the kernel entry recorded by workgroup 0).
  int chk_after() {
#ifdef MPCQ_CHECKED
    int r[16];
    HIP_TRY(hipMemcpyAsync(r, st.chk, sizeof(r), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    if (r[0]) {
      HIP_TRY(hipMemsetAsync(st.chk, 0, sizeof(r), stream));
      const unsigned long long pc = ((unsigned long long)(unsigned)r[8] << 32) | (unsigned)r[7], entry = ((unsigned long long)(unsigned)r[10] << 32) | (unsigned)r[9];
      char buf[320];
      snprintf(buf, sizeof(buf), "checked build: %s tag %d index %d outside [%d, %d) on lane %d of workgroup %d, pc - entry = 0x%llx",
               r[1] >= mpcq::CK_EXEC ? "partial EXEC mask at cross-lane site," : "out-of-range access, region", r[1], r[2], r[3], r[4], r[5], r[6],
               (unsigned long long)(pc - entry));
      return fail(MPCQ_ERR_DEVICE, buf);
    }
#endif
    return 0;
  }
  int base_mode() const { return (cfg.flags & MPCQ_FLAG_STATIC_GP) ? mpcq::MODE_STATIC_GP : 0; }
  // ---- flight recorder (mpcq_record.hpp): the two launches that read the RGP state in the engine's precision
  // in front of the step launch: what compute_a_drag of the step compares against (the post phase overwrites it), selection part [j0, j1)
  void rec_snapshot(hipStream_t s, int j0, int j1) {
    const int n = j1 - j0;
    if (!(rec.fields & MPCQ_RECORD_DRAG) || n <= 0) return;
    hipLaunchKernelGGL(mpcq::record::record_snapshot_kernel, dim3((n * mpcq::record::SNAP + 63) / 64), dim3(64), 0, s, (const int*)rec.d_sel.p, j0, n,
                       (const double*)st.xpp, (const int*)st.has_prev, rec.d_snap.p);
  }
  // behind the step launch, in front of any plant launch: row `row` of every recorded field for the selection part [j0, j1)
  void rec_write(hipStream_t s, int j0, int j1, int row, const double* xmeas) {
    const int n = j1 - j0;
    if (n <= 0) return;
    mpcq::record::Args<T> a;
    std::memset(&a, 0, sizeof(a));
    const long blocks = row_args(a, rec, j0, n, row, xmeas);
    hipLaunchKernelGGL(mpcq::record::record_kernel<T>, dim3((unsigned)blocks), dim3(64), 0, s, a);
  }
  // The arguments of a row launch of the recorder or the black box (r: either; both keep fields, count, d_sel, d_f, d_solver, d_snap) for
  // the selection part [j0, j0 + n) and write position `row`; returns the blocks of the launch.
  template <typename R> long row_args(mpcq::record::Args<T>& a, const R& r, int j0, int n, int row, const double* xmeas) {
    a.sel = r.d_sel.p; a.j0 = j0; a.n = n; a.count = r.count; a.row = row;
    long blocks = 0;
    for (int f = 0; f < mpcq::record::NF; ++f) {
      a.blk[f] = (int)blocks;
      if (r.fields >> f & 1) blocks += ((long)n * mpcq::record::width(f, nb) + 63) / 64;
    }
    a.blk[mpcq::record::NF] = (int)blocks;
    for (int f = 0; f < mpcq::record::NF - 1; ++f) a.out[f] = r.d_f[f].p;
    a.solver = r.d_solver.p; a.snap = r.d_snap.p;
    a.xmeas = xmeas; a.w = st.w; a.xpred = st.xpred; a.cost = st.cost; a.traj = st.traj;
    a.tlen = st.tlen; a.idx = st.idx; a.finished = st.finished; a.status = st.status; a.qp_iter = st.qp_iter;
    a.mu = st.mu; a.C = st.C;
    a.Tmax = m.Tmax; a.N = N; a.skip = m.skip; a.nb = nb; a.dt_pred = m.dt_pred;
    return blocks;
  }
  // ---- incident recorder (mpcq_blackbox.hpp), selection part [j0, j1).  In front of the step launch, behind the recorder's snapshot: the
  // black box's own snapshot
  void bb_snapshot(hipStream_t s, int j0, int j1) {
    const int n = j1 - j0;
    if (!(bb.fields & MPCQ_RECORD_DRAG) || n <= 0) return;
    hipLaunchKernelGGL(mpcq::record::record_snapshot_kernel, dim3((n * mpcq::record::SNAP + 63) / 64), dim3(64), 0, s, (const int*)bb.d_sel.p, j0, n,
                       (const double*)st.xpp, (const int*)st.has_prev, bb.d_snap.p);
  }
  // behind the recorder's row, in front of the score: period `per` into ring slot `slot` of whoever is not frozen, then the judge (judged:
  // what it judges -- the measurement, or under MPCQ_SENSOR_JUDGE_TRUTH the plant state)
  void bb_write(hipStream_t s, int j0, int j1, int slot, long long per, const double* xmeas, const double* judged) {
    namespace bx = mpcq::blackbox;
    const int n = j1 - j0;
    if (n <= 0) return;
    bx::RowArgs<T> a;
    std::memset(&a, 0, sizeof(a));
    const long blocks = row_args(a, bb, j0, n, slot, xmeas);
    a.state = bb.state().state;
    hipLaunchKernelGGL(bx::row_kernel<T>, dim3((unsigned)blocks), dim3(64), 0, s, a);
    bx::JudgeArgs g;
    g.sel = bb.d_sel.p; g.j0 = j0; g.n = n; g.rules = bb.d_rules.p; g.st = bb.state();
    g.period = per; g.post = bb.post;
    g.xmeas = judged; g.w = st.w; g.cost = st.cost; g.traj = st.traj;
    g.tlen = st.tlen; g.idx = st.idx; g.status = st.status; g.qp_iter = st.qp_iter;
    g.Tmax = m.Tmax; g.N = N; g.skip = m.skip;
    hipLaunchKernelGGL(bx::judge_kernel, dim3((n + 63) / 64), dim3(64), 0, s, g);
  }
  // The plant update of the quadrotors [b0, b0 + n): n_sub substeps of sim_dt on xs [B,13] with the controls st.w.  The engine's shared plant
  // (plant_kernel, which reads the model in the engine's precision), or with a fleet set (fper >= 0: its fleet period) every quadrotor's own
  // (fleet_launch).  The one place a plant update is launched.
  void plant_launch(hipStream_t s, int b0, int n, double* xs, int n_sub, double sim_dt, long long fper) {
    if (fper >= 0) return fleet_launch(fl, view(), B, s, b0, n, xs, n_sub, sim_dt, fper);
    hipLaunchKernelGGL(mpcq::plant_kernel<T>, dim3((n + 63) / 64), dim3(64), 0, s, m, xs + (size_t)b0 * 13, st.w + (size_t)b0 * 4, n_sub, sim_dt, n);
  }
  // one lockstep period of the quadrotors [b0, b0 + nq) on stream `strm`; ev_begin (if any) is recorded in front of the STEP kernel, behind
  // the ordering launch, so that the event pairs of sim_steps time the step kernel alone
  void launch_period(const mpcq::DevState<T>& s, int mode, hipEvent_t ev_begin, hipStream_t strm, int b0, int nq) {
    mpcq::DevState<T> so = s;
    so.b0 = b0;
    if (use_order) {   // (reads qp_iter of the previous period; a permutation by construction whatever qp_iter holds: order_bin is total)
      hipLaunchKernelGGL(mpcq::order_kernel, dim3(mpcq::ORD_CLASSES), dim3(mpcq::ORD_THREADS), mpcq::ORD_LDS, strm, (const int*)st.qp_iter + b0, nq, d_order + b0, b0);
      so.order = d_order + b0;
    }
    if (ev_begin) (void)hipEventRecord(ev_begin, strm);
    hipLaunchKernelGGL(kstep, dim3(nq), dim3(64), lds_bytes, strm, m, so, mode);
  }
  // The optional events of a period (see period)
  struct PeriodEvents { hipEvent_t front = nullptr, step = nullptr, end = nullptr; };
  // One period of groups[gi], the only place that issues one.  On the group's stream, in this order:
  //   the sensor's launch (t.nper >= 0: the period measures through the sensor; s.x_meas is its output then) -> the recorder's snapshot (t.row >= 0: the period is recorded) -> the black box's snapshot (t.bslot >= 0: a black box runs) -> ev.front
  //   -> ordering launch -> ev.step -> step kernel -> ev.end -> the recorder's row -> the black box's row and judge launches
  //   -> the scoreboard's launch (t.sper >= 0) -> the exploration launch (an exploration runs and t.mper >= 0)
  //   -> the plant update (plant: s.run_nsub substeps of s.run_dt on s.run_x; with t.fper >= 0 the fleet's launch, plant_launch)
  //   -> the mission launch (t.mper >= 0; the flights start at the plant state behind its update, or without a plant at the period's
  //   measurement).
  // Under MPCQ_SENSOR_JUDGE_TRUTH the scoreboard and the black box's judge read the plant state (judged) where the rows read s.x_meas.
  // The caller asks hipGetLastError once it has issued all it has to issue.
  int period(int gi, const mpcq::DevState<T>& s, int mode, const Tick& t, const PeriodEvents& ev, bool plant) {
    const Group& g = groups[gi];
    if (g.n <= 0) return 0;
    const EngineView v = view();
    const double* judged = sn.on && sn.judge == MPCQ_SENSOR_JUDGE_TRUTH ? v.plant : s.x_meas;
    if (t.nper >= 0) sensor_launch(sn, v, B, g.stream, g.b0, g.n, t.nper);
    if (t.row >= 0) rec_snapshot(g.stream, rec.glo[gi], rec.ghi[gi]);
    if (t.bslot >= 0) bb_snapshot(g.stream, bb.glo[gi], bb.ghi[gi]);
    if (ev.front) HIP_TRY(hipEventRecord(ev.front, g.stream));
    launch_period(s, mode, ev.step, g.stream, g.b0, g.n);
    if (ev.end) HIP_TRY(hipEventRecord(ev.end, g.stream));
    if (t.row >= 0) rec_write(g.stream, rec.glo[gi], rec.ghi[gi], t.row, s.x_meas);
    if (t.bslot >= 0) bb_write(g.stream, bb.glo[gi], bb.ghi[gi], t.bslot, t.bper, s.x_meas, judged);
    if (t.sper >= 0) score_launch(sc, v, B, g.stream, g.b0, g.n, t.sper, judged);
    if (ex.on && t.mper >= 0) explore_launch(ex, ms, v, B, g.stream, g.b0, g.n, s.x_meas);
    if (plant) plant_launch(g.stream, g.b0, g.n, s.run_x, s.run_nsub, s.run_dt, t.fper);
    if (t.mper >= 0) mission_launch(ms, v, B, g.stream, g.b0, g.n, plant ? s.run_x : s.x_meas, t.mper);
    return 0;
  }
  int solve(const double* x0) override {
    int rc;
    if ((rc = h2d(d_xin, x0, (size_t)B * 13))) return rc;
    st.x_meas = d_xin;
    if ((rc = period(n_groups, st, 0, Tick{}, PeriodEvents{ev0, nullptr, ev1}, false))) return rc;
    HIP_TRY(hipGetLastError());
    timed = true;
    HIP_TRY(hipStreamSynchronize(stream));
    return chk_after();
  }
  // rows [B][width] of `stage` out of src [B][stages][width]: one strided copy (a reference-shaped `for i: get(i,'x')` loop stays O(N B))
  int get_stage(const double* src, size_t width, int stages, int stage, double* out) {
    if (stage < 0 || stage >= stages) return fail(MPCQ_ERR_INVALID, "stage out of range");
    HIP_TRY(hipMemcpy2DAsync(out, width * sizeof(double), src + stage * width, stages * width * sizeof(double), width * sizeof(double), B, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return 0;
  }
  int get_x(int stage, double* out) override { return get_stage(st.X, 13, N + 1, stage, out); }
  int get_u(int stage, double* out) override { return get_stage(st.U, 4, N, stage, out); }
  int get_cost(double* out) override { return d2h(out, st.cost, B); }
  int get_int(int which, int32_t* out) override {
    const int* src = which == 0 ? st.status : (which == 1 ? st.qp_iter : (which == 2 ? st.idx : (which == 4 ? st.qp_work : (which == 5 ? st.finished : st.has_prev))));
    return copy_sync(out, src, (size_t)B * sizeof(int), hipMemcpyDeviceToHost);
  }
  int predict(const double* x, const double* u, double dt, double* out) override {
    int rc;
    if ((rc = h2d(d_xin, x, (size_t)B * 13))) return rc;
    if ((rc = h2d(d_uin, u, (size_t)B * 4))) return rc;
    hipLaunchKernelGGL(mpcq::predict_kernel<T>, dim3((B + 63) / 64), dim3(64), 0, stream, m, d_xin, d_uin, dt, d_tmp, B);
    HIP_TRY(hipGetLastError());
    return d2h(out, d_tmp, (size_t)B * 13);
  }
  int regress(const double* vb, const double* ad) override {
    if (!nb) return fail(MPCQ_ERR_STATE, "engine has no RGP (nb = 0)");
    int rc;
    if ((rc = h2d(d_vb, vb, (size_t)B * 3))) return rc;
    if ((rc = h2d(d_ad, ad, (size_t)B * 3))) return rc;
    hipLaunchKernelGGL(mpcq::regress_kernel<T>, dim3(B), dim3(64), lds_bytes, stream, m, st, d_vb, d_ad);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(stream));
    return chk_after();
  }
  int get_rgp(double* mu, double* C) override {
    int rc;
    if (mu && nb && (rc = q2h(mu, st.mu, (size_t)B * 3 * nb))) return rc;
    if (C && nb && (rc = q2h(C, st.C, (size_t)B * 3 * nb * nb))) return rc;
    return 0;
  }
  // the live model: the static GP's posterior has no J C J^T term and does not read C (src/gp/GP.py:135-179)
  int rgp_predict(const double* xq, int M, int per_quad, double* mean, double* var) override {
    const bool fixed = (cfg.flags & MPCQ_FLAG_STATIC_GP) != 0;
    return predict_run<T>(this, st.mu, 3L * nb, fixed ? nullptr : st.C, 3L * nb * nb, (size_t)B, nullptr, 0, 1, B, xq, M, per_quad, mean, var);
  }
  int step(const double* x_meas, double* w_out, double* x_pred_out) override {
    if (const int rc = needs_trajectories(this, "mpcq_step")) return rc;
    // host buffers go through one pinned staging block so that the three copies are truly asynchronous and the
    // call synchronises once: H2D x_meas -> step kernel -> D2H w, x_pred
    const size_t nx = (size_t)B * 13, nw = (size_t)B * 4;
    if (!h_pin) HIP_TRY(hipHostMalloc((void**)&h_pin, (2 * nx + nw) * sizeof(double), hipHostMallocDefault));
    std::memcpy(h_pin, x_meas, nx * sizeof(double));
    HIP_TRY(hipMemcpyAsync(d_xin, h_pin, nx * sizeof(double), hipMemcpyHostToDevice, stream));
    st.x_meas = d_xin;
    int rc;
    if ((rc = period(n_groups, st, mpcq::MODE_TRAJ | mpcq::MODE_POST | base_mode(), next_tick(true, false), PeriodEvents{ev0, nullptr, ev1}, false))) return rc;
    HIP_TRY(hipGetLastError());
    timed = true;
    HIP_TRY(hipMemcpyAsync(h_pin + nx, st.w, nw * sizeof(double), hipMemcpyDeviceToHost, stream));
    if (x_pred_out) HIP_TRY(hipMemcpyAsync(h_pin + nx + nw, st.xpred, nx * sizeof(double), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    std::memcpy(w_out, h_pin + nx, nw * sizeof(double));
    if (x_pred_out) std::memcpy(x_pred_out, h_pin + nx + nw, nx * sizeof(double));
    return chk_after();
  }
  int step_device(const double* d_x, double* d_w) override {
    if (const int rc = needs_trajectories(this, "mpcq_step_device_async")) return rc;
    mpcq::DevState<T> s2 = st;   // measurement and control are float64 in every precision (DevState::x_meas / w)
    s2.x_meas = d_x;
    s2.w_ext = d_w;   // the engine's own control record st.w is written as well (mpcq_get_command, mpcq_sim_plant_period(w = NULL))
    int rc;
    if ((rc = period(n_groups, s2, mpcq::MODE_TRAJ | mpcq::MODE_POST | base_mode(), next_tick(true, false), PeriodEvents{ev0, nullptr, ev1}, false))) return rc;
    HIP_TRY(hipGetLastError());
    timed = true;
    return chk_after();   // (synchronises in the checked build only)
  }
  int sim_reset(const double* x0) override { return h2d(d_xs, x0, (size_t)B * 13); }
  int sim_steps(int K, int n_sub, double sim_dt) override {
    if (const int rc = needs_trajectories(this, "mpcq_sim_steps")) return rc;
    mpcq::DevState<T> s2 = st;
    s2.x_meas = sn.on ? sn.out(B) : d_xs;   // (a sensor's launch in front of every period turns d_xs into its output)
    // HIP events around every 4th step-kernel launch: an event pair between two dependent launches costs dispatch overlap (measured
    // at B = 1 024, 20 launches: pairs on every launch 3.18 M steps/s, on every 2nd 3.22, every 4th 3.25, none 3.26), so only a sample of
    // the launches carries one (calls of fewer than 8 periods: every launch; MPCQ_KEV_STRIDE under MPCQ_TUNING=1 overrides)
    int stride = K < 8 ? 1 : 4;
    if (const char* t = tuning_env ? getenv("MPCQ_KEV_STRIDE") : nullptr) stride = atoi(t) > 0 ? atoi(t) : 1;
    const int nev = (K + stride - 1) / stride;
    while ((int)kev.size() < 2 * nev) { hipEvent_t ev; HIP_TRY(hipEventCreate(&ev)); kev.push_back(ev); }
    HIP_TRY(hipEventRecord(ev0, stream));
    // The plant update between two control periods rides at the head of the next step launch (MODE_PLANT_FIRST), where
    // it overlaps that launch's global loads; only the update after the last period needs the plant kernel.  Streaming batches
    // (split_plant, see create): every update is a launch of the plant kernel.  Same arithmetic, same results either way.
    // An active mission plans from the plant state behind the period's update, so it needs that update in front of its launch: every
    // update is a launch then, too.  A fleet's plants are integrated by a kernel of their own (mpcq_fleet.hpp): every update is its launch.
    // A sensor measures the plant state in front of the step (MODE_PLANT_FIRST would measure from the buffer it is about to integrate): every
    // update is a launch then, too.
    const bool split = split_plant || ms.on || fl.on || sn.on;
    s2.run_x = d_xs; s2.run_steps = 1; s2.run_nsub = n_sub; s2.run_dt = sim_dt;
    // Groups (see init): the K periods {order, step, plant} of a group go to its stream, issued period by period round the groups so that
    // the host feeds every queue.  The group streams start behind everything issued on the engine's stream and the engine's stream
    // continues behind all of them; a batch that is one group runs on the engine's stream and needs neither.  Event pairs: group 0's
    // launches (with more groups, a launch of B / G quadrotors that shares the device).
    const int G = n_groups;
    if (G > 1) HIP_TRY(hipEventRecord(gstart, stream));
    for (int g = 1; g < G; ++g) HIP_TRY(hipStreamWaitEvent(groups[g].stream, gstart, 0));
    int rc;
    for (int k = 0; k < K; ++k) {
      const Tick tick = next_tick(true, true, true);   // (one ticket per control period, the same for every group: the recorder's launches of a group cover the selection inside it)
      const int mode = mpcq::MODE_TRAJ | mpcq::MODE_POST | base_mode() | ((!split && k > 0) ? mpcq::MODE_PLANT_FIRST : 0);
      for (int g = 0; g < G; ++g) {
        PeriodEvents ev;
        if (g == 0 && k % stride == 0) { ev.step = kev[2 * (k / stride)]; ev.end = kev[2 * (k / stride) + 1]; }
        if ((rc = period(g, s2, mode, tick, ev, split || k == K - 1))) return rc;
      }
    }
    for (int g = 1; g < G; ++g) {
      HIP_TRY(hipEventRecord(groups[g].done, groups[g].stream));
      HIP_TRY(hipStreamWaitEvent(stream, groups[g].done, 0));
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(ev1, stream));
    timed = true;
    HIP_TRY(hipStreamSynchronize(stream));
    ktime = 0; kmin = 1e30; kmax = 0;
    klaunches = nev;
    for (int k = 0; k < nev; ++k) {
      float ms = 0;
      HIP_TRY(hipEventElapsedTime(&ms, kev[2 * k], kev[2 * k + 1]));
      ktime += ms * 1e-3;
      kmin = std::min(kmin, (double)ms * 1e-3); kmax = std::max(kmax, (double)ms * 1e-3);
    }
    if (!nev) kmin = 0;
    return chk_after();
  }
  int sim_run(int K, int n_sub, double sim_dt) override {
    if (const int rc = needs_trajectories(this, "mpcq_sim_run")) return rc;
    if (rec.on) return fail(MPCQ_ERR_STATE, "mpcq_sim_run cannot record (one persistent launch): mpcq_record_stop first, or use mpcq_sim_steps");
    if (bb.on) return fail(MPCQ_ERR_STATE, "mpcq_sim_run cannot keep a black box (one persistent launch): mpcq_blackbox_stop first, or use mpcq_sim_steps");
    if (ex.on) return fail(MPCQ_ERR_STATE, "mpcq_sim_run cannot explore (one persistent launch): mpcq_explore_stop and mpcq_mission_stop first, or use mpcq_sim_steps");
    if (ms.on) return fail(MPCQ_ERR_STATE, "mpcq_sim_run cannot fly a mission (one persistent launch): mpcq_mission_stop first, or use mpcq_sim_steps");
    if (sc.on) return fail(MPCQ_ERR_STATE, "mpcq_sim_run cannot score flights (one persistent launch): mpcq_score_stop first, or use mpcq_sim_steps");
    if (fl.on) return fail(MPCQ_ERR_STATE, "mpcq_sim_run cannot fly a fleet (one persistent launch): mpcq_fleet_stop first, or use mpcq_sim_steps");
    if (sn.on) return fail(MPCQ_ERR_STATE, "mpcq_sim_run cannot measure through a sensor (one persistent launch): mpcq_sensor_stop first, or use mpcq_sim_steps");
    if (K <= 0) return 0;
    mpcq::DevState<T> s2 = st;
    s2.x_meas = d_xs;
    s2.run_x = d_xs; s2.run_steps = K; s2.run_nsub = n_sub; s2.run_dt = sim_dt;
    while ((int)kev.size() < 2) { hipEvent_t ev; HIP_TRY(hipEventCreate(&ev)); kev.push_back(ev); }
    HIP_TRY(hipEventRecord(ev0, stream));
    HIP_TRY(hipEventRecord(kev[0], stream));
    hipLaunchKernelGGL(krun, dim3(B), dim3(64), lds_bytes, stream, m, s2, mpcq::MODE_TRAJ | mpcq::MODE_POST | mpcq::MODE_RUN | base_mode());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(kev[1], stream));
    HIP_TRY(hipEventRecord(ev1, stream));
    timed = true;
    HIP_TRY(hipStreamSynchronize(stream));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, kev[0], kev[1]));
    ktime = kmin = kmax = ms * 1e-3;
    klaunches = 1;
    return chk_after();
  }
  int sim_get(double* x, double* w) override {
    int rc;
    if ((rc = d2h(x, d_xs, (size_t)B * 13))) return rc;
    if (w && (rc = d2h(w, st.w, (size_t)B * 4))) return rc;
    return 0;
  }
  int stats(double* out5) override {
    hipLaunchKernelGGL(mpcq::stats_kernel, dim3(1), dim3(256), 5 * 256 * sizeof(double), stream, st.stats, st.status, B, d_stats5);
    HIP_TRY(hipGetLastError());
    if (out5) {
      HIP_TRY(hipMemcpyAsync(out5, d_stats5, 5 * sizeof(double), hipMemcpyDeviceToHost, stream));
      HIP_TRY(hipStreamSynchronize(stream));
    }
    return 0;
  }
  int get_command(double* rotor, double* coll, double* rates) override {
    int rc;
    HIP_TRY(d_cmd.grow((size_t)B * 8));
    double* c = d_cmd.p;
    hipLaunchKernelGGL(mpcq::command_kernel<T>, dim3((B + 63) / 64), dim3(64), 0, stream, m, st.w, st.X, c, c + (size_t)B * 4, c + (size_t)B * 5, B);
    HIP_TRY(hipGetLastError());
    if (rotor && (rc = d2h(rotor, c, (size_t)B * 4))) return rc;
    if (coll && (rc = d2h(coll, c + (size_t)B * 4, (size_t)B))) return rc;
    if (rates && (rc = d2h(rates, c + (size_t)B * 5, (size_t)B * 3))) return rc;
    return 0;
  }
  int get_finished(int32_t* out) override { return get_int(5, out); }
  int get_chunk(double* out) override {
    if (const int rc = needs_trajectories(this, "mpcq_get_reference_chunk")) return rc;
    HIP_TRY(d_cmd.grow((size_t)B * N * 13));
    hipLaunchKernelGGL(mpcq::chunk_kernel<T>, dim3(B), dim3(64), 0, stream, m, st.traj, st.tlen, st.idx, d_cmd.p);
    HIP_TRY(hipGetLastError());
    return d2h(out, d_cmd.p, (size_t)B * N * 13);
  }
  int sim_plant(const double* w, int n_sub, double sim_dt) override {
    int rc;
    if (w && (rc = h2d(st.w, w, (size_t)B * 4))) return rc;
    plant_launch(stream, 0, B, d_xs, n_sub, sim_dt, next_tick(false, true).fper);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(stream));
    return 0;
  }
  int get_solver_state(int32_t* qp_iter, double* stats4, int32_t* finished) override {
    int rc;
    if (qp_iter && (rc = get_int(1, qp_iter))) return rc;
    if (stats4 && (rc = d2h(stats4, st.stats, (size_t)B * 4))) return rc;
    if (finished && (rc = get_finished(finished))) return rc;
    return 0;
  }
  int set_solver_state(const int32_t* qp_iter, const double* stats4, const int32_t* finished) override {
    int rc;
    if (qp_iter)   // decimal fields of include/mpcq.h: passes < 1000, three one-digit fields above
      for (int b = 0; b < B; ++b)
        if (qp_iter[b] < 0 || qp_iter[b] >= 1000000) return fail(MPCQ_ERR_INVALID, "mpcq_set_solver_state: qp_iter outside [0, 1e6)");
    if (finished)
      for (int b = 0; b < B; ++b)
        if (finished[b] != 0 && finished[b] != 1) return fail(MPCQ_ERR_INVALID, "mpcq_set_solver_state: finished must be 0 or 1");
    if (qp_iter) HIP_TRY(hipMemcpyAsync(st.qp_iter, qp_iter, (size_t)B * sizeof(int), hipMemcpyHostToDevice, stream));
    if (finished) HIP_TRY(hipMemcpyAsync(st.finished, finished, (size_t)B * sizeof(int), hipMemcpyHostToDevice, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    if (stats4 && (rc = h2d(st.stats, stats4, (size_t)B * 4))) return rc;
    return 0;
  }
  int get_order(int32_t* out) override {   // the permutation the last lockstep launch used (identity when no order is in use)
    if (!use_order) { for (int b = 0; b < B; ++b) out[b] = b; return 0; }
    return copy_sync(out, d_order, (size_t)B * sizeof(int), hipMemcpyDeviceToHost);
  }
  int get_prof(unsigned long long* out) override {
#if defined(MPCQ_PROFILE) || defined(MPCQ_TRACE_NAN)
    HIP_TRY(hipMemcpyAsync(out, st.prof, (size_t)B * mpcq::PF_N * sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return 0;
#else
    (void)out;
    return fail(MPCQ_ERR_STATE, "built without MPCQ_PROFILE");
#endif
  }
  int get_state(double* X, double* U, double* mu, double* C, double* xpp, int32_t* hp, int32_t* idx) override {
    int rc;
    if (X && (rc = d2h(X, st.X, (size_t)B * (N + 1) * 13))) return rc;
    if (U && (rc = d2h(U, st.U, (size_t)B * N * 4))) return rc;
    if ((rc = get_rgp(mu, C))) return rc;
    if (xpp && (rc = d2h(xpp, st.xpp, (size_t)B * 13))) return rc;
    if (hp && (rc = get_int(3, hp))) return rc;
    if (idx && (rc = get_int(2, idx))) return rc;
    return 0;
  }
  int set_state(const double* X, const double* U, const double* mu, const double* C, const double* xpp, const int32_t* hp,
                const int32_t* idx) override {
    int rc;
    // a negative cursor would make the step kernel read reference rows in front of its trajectory (only the checked build would
    // notice): refused here.  A cursor at or beyond the end is legal (get_reference_chunk repeats the last row, src/utils/utils.py:897-931).
    const bool unchecked = tuning_env && getenv("MPCQ_SKIP_STATE_CHECKS");   // tests of the checked build provoke a violation this way
    if (idx && !unchecked)
      for (int b = 0; b < B; ++b)
        if (idx[b] < 0) return fail(MPCQ_ERR_INVALID, "mpcq_set_state: negative trajectory cursor");
    if (hp)
      for (int b = 0; b < B; ++b)
        if (hp[b] != 0 && hp[b] != 1) return fail(MPCQ_ERR_INVALID, "mpcq_set_state: has_prev must be 0 or 1");
    if (X && (rc = h2d(st.X, X, (size_t)B * (N + 1) * 13))) return rc;
    if (U && (rc = h2d(st.U, U, (size_t)B * N * 4))) return rc;
    if (mu && nb && (rc = h2q(st.mu, mu, (size_t)B * 3 * nb))) return rc;
    if (C && nb && (rc = h2q(st.C, C, (size_t)B * 3 * nb * nb))) return rc;
    if (xpp && (rc = h2d(st.xpp, xpp, (size_t)B * 13))) return rc;
    if (hp) HIP_TRY(hipMemcpyAsync(st.has_prev, hp, (size_t)B * sizeof(int), hipMemcpyHostToDevice, stream));
    if (idx) HIP_TRY(hipMemcpyAsync(st.idx, idx, (size_t)B * sizeof(int), hipMemcpyHostToDevice, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return 0;
  }
};

}  // namespace

// ------------------------------------------------------------------ C ABI
extern "C" {

const char* mpcq_last_error(void) { return g_err.c_str(); }
#ifndef MPCQ_SRC_ID   // csrc/Makefile: the first 16 hex digits of sha256(mpcq_kernels.hpp | mpcq_api.hip | mpcq_spec.hip | Makefile | cc_checked.sh) = bench.kernel_source_sha16()
#define MPCQ_SRC_ID "unknown"
#endif
#ifdef MPCQ_CHECKED
const char* mpcq_version(void) { return "mpcq 0.6.7 (gfx950, CHECKED diagnostic build, source " MPCQ_SRC_ID ")"; }
#else
const char* mpcq_version(void) { return "mpcq 0.6.7 (gfx950, source " MPCQ_SRC_ID ")"; }
#endif

// binaries built against the 0.3 header (source callers get the header's inline, which passes their own sizeof): the 0.3 layout ends
// in front of mpcq_tuning.block_order
int mpcq_create(const mpcq_config* c, mpcq_engine** out) { return mpcq_create_sized(c, offsetof(mpcq_config, tune) + offsetof(mpcq_tuning, block_order), out); }
int mpcq_create_sized(const mpcq_config* c_in, uint64_t cfg_size, mpcq_engine** out) {
  if (!c_in || !out) return fail(MPCQ_ERR_INVALID, "null argument");
  *out = nullptr;
  // fields behind the caller's struct size take their defaults (0); everything up to and including `flags` is required
  if (cfg_size < offsetof(mpcq_config, finish_radius) || cfg_size > sizeof(mpcq_config))
    return fail(MPCQ_ERR_INVALID, "mpcq_config size not understood by this library (built against a different mpcq.h?)");
  mpcq_config cc;
  std::memset(&cc, 0, sizeof(cc));
  std::memcpy(&cc, c_in, (size_t)cfg_size);
  const mpcq_config* c = &cc;
  if (c->batch <= 0 || c->N < 2 || c->N > 128 || c->nb < 0 || c->nb > 128 || c->skip < 1 || !(c->T > 0) || !(c->dt_pred > 0))
    return fail(MPCQ_ERR_INVALID, "bad batch/N/nb/skip/T/dt_pred");
  if (c->nb > 0 && (!c->basis || !c->theta)) return fail(MPCQ_ERR_INVALID, "nb > 0 needs basis and theta");
  if (!(c->mass > 0) || !(c->J[0] > 0) || !(c->J[1] > 0) || !(c->J[2] > 0)) return fail(MPCQ_ERR_INVALID, "bad mass/inertia");
  for (int i = 0; i < 4; ++i)
    if (!(c->u_ub[i] > c->u_lb[i])) return fail(MPCQ_ERR_INVALID, "u_ub must exceed u_lb");
  for (int i = 13; i < 17; ++i)
    if (!(c->W[i] > 0)) return fail(MPCQ_ERR_INVALID, "input weights must be positive (strictly convex QP)");
  if (!(c->finish_radius >= 0)) return fail(MPCQ_ERR_INVALID, "finish_radius must be >= 0 (0 = default 1 m)");
  if (!(c->qp_tol >= 0) || c->qp_tol > 1e-1) return fail(MPCQ_ERR_INVALID, "qp_tol out of range [0, 1e-1]");
  if (c->qp_max_iter < 0 || c->qp_max_iter > 500) return fail(MPCQ_ERR_INVALID, "qp_max_iter out of range [0, 500]");
  {
    const mpcq_tuning& t = c->tune;
    auto irange = [](int v, int lo, int hi, bool neg1) { return v == 0 || (neg1 && v == -1) || (v >= lo && v <= hi); };
    auto frange = [](double v, double lo, double hi) { return v == 0 || (v >= lo && v <= hi); };   // NaN fails both
    if (!irange(t.warm_max, 1, 64, false) || !irange(t.warm_retry, 1, 64, false) || !irange(t.flip_max, 1, 512, true) ||
        !irange(t.abort_pins, 1, 512, true) || !irange(t.abort_wrong, 1, 512, true) || !irange(t.polish_max, 1, 64, true) ||
        !irange(t.stage_mem, 1, 3, false) || !irange(t.generic_kernel, 1, 1, false) || !irange(t.block_order, 1, 2, false) || !irange(t.groups, 1, 16, false))
      return fail(MPCQ_ERR_INVALID, "mpcq_config.tune: integer field out of range (see mpcq.h)");
    // MPCQ_PRECISION_F32 answers from the active-set method (iterate and residuals in double); without it every fallback solve would return
    // the float interior point's own answer with MPCQ_SOLVE_LOW_ACCURACY and the 1e-4 budget would not hold
    if (c->precision == MPCQ_PRECISION_F32 && t.polish_max == -1)
      return fail(MPCQ_ERR_INVALID, "mpcq_config.tune.polish_max = -1 (no active-set passes) is not available with MPCQ_PRECISION_F32");
    if (!frange(t.pin_ratio, 1e-300, 1e3) || !frange(t.ipm_mu0, 1e-12, 1.0) || !(t.ipm_margin == 0 || (t.ipm_margin > 0 && t.ipm_margin < 0.5)) ||
        !frange(t.ipm_tol, 1e-300, 1e-1))
      return fail(MPCQ_ERR_INVALID, "mpcq_config.tune: real field out of range (see mpcq.h)");
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(MPCQ_ERR_DEVICE, "no HIP device: libmpcq has no CPU path (the CPU restatement lives in oracle/ for tests only)");
  if (c->device < 0 || c->device >= ndev) return fail(MPCQ_ERR_INVALID, "device ordinal out of range");
  DeviceGuard guard(c->device);
  mpcq_engine* e = nullptr;
  if (c->precision == MPCQ_PRECISION_F64) e = new EngineT<double>();
  else if (c->precision == MPCQ_PRECISION_F32) e = new EngineT<float>();
  else return fail(MPCQ_ERR_INVALID, "unknown precision");
  e->cfg = *c;
  e->B = c->batch; e->N = c->N; e->nb = c->nb;
  if (c->nb) { e->basis.assign(c->basis, c->basis + 3 * c->nb); e->theta.assign(c->theta, c->theta + 9); }
  e->cfg.basis = nullptr; e->cfg.theta = nullptr;
  const int rc = e->init();
  if (rc) { delete e; return rc; }   // (under `guard`)
  *out = e;
  return 0;
}
// (the guard outlives the destructors of the engine's members, which free its device memory)
int mpcq_destroy(mpcq_engine* e) { if (!e) return 0; DeviceGuard guard(e->cfg.device); delete e; return 0; }
// null check + the engine's device made current for the duration of the call
#define ENTER(e) if (!(e)) return fail(MPCQ_ERR_INVALID, "null engine"); DeviceGuard guard_((e)->cfg.device)
int mpcq_reset(mpcq_engine* e) { ENTER(e); return e->reset(); }
int mpcq_set_trajectories(mpcq_engine* e, const double* t, const int32_t* len, int32_t Tmax) { ENTER(e); if (!t || !len) return fail(MPCQ_ERR_INVALID, "null argument"); return e->set_trajectories(t, len, Tmax); }
int mpcq_set_reference(mpcq_engine* e, const double* y, const double* yN) { ENTER(e); if (!y || !yN) return fail(MPCQ_ERR_INVALID, "null argument"); return e->set_reference(y, yN); }
int mpcq_set_params(mpcq_engine* e, const double* mu) { ENTER(e); if (!mu && e->nb) return fail(MPCQ_ERR_INVALID, "null argument"); return e->set_params(mu); }
int mpcq_solve(mpcq_engine* e, const double* x0) { ENTER(e); if (!x0) return fail(MPCQ_ERR_INVALID, "x_init has to be set before running the optimization"); return e->solve(x0); }
int mpcq_get_x(mpcq_engine* e, int32_t s, double* o) { ENTER(e); return e->get_x(s, o); }
int mpcq_get_u(mpcq_engine* e, int32_t s, double* o) { ENTER(e); return e->get_u(s, o); }
int mpcq_get_cost(mpcq_engine* e, double* o) { ENTER(e); return e->get_cost(o); }
int mpcq_get_status(mpcq_engine* e, int32_t* o) { ENTER(e); return e->get_int(0, o); }
int mpcq_get_qp_iter(mpcq_engine* e, int32_t* o) { ENTER(e); return e->get_int(1, o); }
int mpcq_get_qp_work(mpcq_engine* e, int32_t* o) { ENTER(e); if (!o) return fail(MPCQ_ERR_INVALID, "null argument"); return e->get_int(4, o); }
int mpcq_get_stats(mpcq_engine* e, double* t) {
  ENTER(e);
  if (e->timed) {
    float ms = 0;
    if (hipEventSynchronize(e->ev1) == hipSuccess && hipEventElapsedTime(&ms, e->ev0, e->ev1) == hipSuccess) e->last_time = ms * 1e-3;
  }
  if (t) *t = e->last_time;
  return 0;
}
int mpcq_predict_nominal(mpcq_engine* e, const double* x, const double* u, double dt, double* o) { ENTER(e); return e->predict(x, u, dt, o); }
int mpcq_rgp_regress(mpcq_engine* e, const double* vb, const double* ad) { ENTER(e); return e->regress(vb, ad); }
int mpcq_get_rgp(mpcq_engine* e, double* mu, double* C) { ENTER(e); return e->get_rgp(mu, C); }
int mpcq_step(mpcq_engine* e, const double* x, double* w, double* xp) { ENTER(e); if (!x || !w) return fail(MPCQ_ERR_INVALID, "null argument"); return e->step(x, w, xp); }
int mpcq_step_device_async(mpcq_engine* e, const double* dx, double* dw) { ENTER(e); if (!dx) return fail(MPCQ_ERR_INVALID, "null argument"); return e->step_device(dx, dw); }
int mpcq_synchronize(mpcq_engine* e) { ENTER(e); HIP_TRY(hipStreamSynchronize(e->stream)); return 0; }
void* mpcq_stream(mpcq_engine* e) { return e ? (void*)e->stream : nullptr; }
int mpcq_get_command(mpcq_engine* e, double* rotor, double* coll, double* rates) { ENTER(e); return e->get_command(rotor, coll, rates); }
int mpcq_get_finished(mpcq_engine* e, int32_t* o) { ENTER(e); if (!o) return fail(MPCQ_ERR_INVALID, "null argument"); return e->get_finished(o); }
int mpcq_get_reference_chunk(mpcq_engine* e, double* o) { ENTER(e); if (!o) return fail(MPCQ_ERR_INVALID, "null argument"); return e->get_chunk(o); }
int mpcq_sim_reset(mpcq_engine* e, const double* x0) {
  ENTER(e);
  const int rc = e->sim_reset(x0);
  if (!rc) e->have_sim = true;
  return rc;
}
int mpcq_sim_steps(mpcq_engine* e, int32_t K, int32_t n_sub, double sim_dt) { ENTER(e); return e->sim_steps(K, n_sub, sim_dt); }
int mpcq_sim_run(mpcq_engine* e, int32_t K, int32_t n_sub, double sim_dt) { ENTER(e); return e->sim_run(K, n_sub, sim_dt); }
// `while control_time < optimization_dt: quad.update(w, simulation_dt); control_time += simulation_dt`
// (src/execute_trajectory.py:232-243): the count comes out of the same double accumulation (20 / 11 / 4 at 0.1 / 0.05 / 0.02)
int mpcq_plant_substeps(double control_dt, double sim_dt) {
  if (!(sim_dt > 0) || !(control_dt > 0) || control_dt / sim_dt > 1e6) return -1;
  double t = 0;
  int n = 0;
  while (t < control_dt) { t += sim_dt; ++n; }
  return n;
}
int mpcq_sim_plant_period(mpcq_engine* e, const double* w, double control_dt, double sim_dt, int32_t* n_sub) {
  ENTER(e);
  const int n = mpcq_plant_substeps(control_dt, sim_dt);
  if (n < 0) return fail(MPCQ_ERR_INVALID, "bad control_dt / sim_dt");
  if (n_sub) *n_sub = n;
  return e->sim_plant(w, n, sim_dt);
}
int mpcq_sim_control_periods(mpcq_engine* e, int32_t K, double control_dt, double sim_dt, int32_t* n_sub) {
  ENTER(e);
  const int n = mpcq_plant_substeps(control_dt, sim_dt);
  if (n < 0) return fail(MPCQ_ERR_INVALID, "bad control_dt / sim_dt");
  if (n_sub) *n_sub = n;
  return e->sim_steps(K, n, sim_dt);
}
int mpcq_sim_get_state(mpcq_engine* e, double* x, double* w) { ENTER(e); return e->sim_get(x, w); }
int mpcq_get_kernel_time(mpcq_engine* e, double* s, int32_t* n) { ENTER(e); if (s) *s = e->ktime; if (n) *n = e->klaunches; return 0; }
int mpcq_get_kernel_time_minmax(mpcq_engine* e, double* mn, double* mx) { ENTER(e); if (mn) *mn = e->kmin; if (mx) *mx = e->kmax; return 0; }
int mpcq_get_tracking_stats(mpcq_engine* e, double out[5]) { ENTER(e); return e->stats(out); }
#ifdef MPCQ_DUMP_AT   /* reproducer builds only (tools/repro_codegen; not part of include/mpcq.h): [B][4096] doubles */
int mpcq_debug_dump(mpcq_engine* e, double* out) {
  ENTER(e);
  double* src = e->cfg.precision == MPCQ_PRECISION_F64 ? static_cast<EngineT<double>*>(e)->m.dbg : static_cast<EngineT<float>*>(e)->m.dbg;
  HIP_TRY(hipMemcpy(out, src, (size_t)e->B * 4096 * sizeof(double), hipMemcpyDeviceToHost));
  return 0;
}
#endif
/* diagnostic build only: per-instance phase cycle totals of the last step, [B][16] */
int mpcq_debug_profile(mpcq_engine* e, unsigned long long* out) { ENTER(e); return e->get_prof(out); }
int mpcq_get_groups(mpcq_engine* e, int32_t* out) { ENTER(e); if (!out) return fail(MPCQ_ERR_INVALID, "null argument"); *out = e->n_groups; return 0; }
int mpcq_get_block_order(mpcq_engine* e, int32_t* out) { ENTER(e); if (!out) return fail(MPCQ_ERR_INVALID, "null argument"); return e->get_order(out); }

int mpcq_comm_unique_id(void* id128) {
  int rc = rccl_load();
  if (rc) return rc;
  const int r = g_rccl.GetUniqueId(id128);
  if (r) return fail(MPCQ_ERR_COMM, std::string("ncclGetUniqueId: ") + (g_rccl.GetErrorString ? g_rccl.GetErrorString(r) : "?"));
  return 0;
}
int mpcq_comm_init(mpcq_engine* e, int32_t rank, int32_t nranks, const void* id128) {
  ENTER(e);
  if (!id128 || nranks < 1 || rank < 0 || rank >= nranks) return fail(MPCQ_ERR_INVALID, "bad rank / nranks / id");
  if (e->comm) return fail(MPCQ_ERR_STATE, "communicator already initialised");
  int rc = rccl_load();
  if (rc) return rc;
  Id128 id;
  std::memcpy(&id, id128, sizeof(id));
  const int r = g_rccl.CommInitRank(&e->comm, nranks, id, rank);
  if (r) { e->comm = nullptr; return fail(MPCQ_ERR_COMM, std::string("ncclCommInitRank: ") + (g_rccl.GetErrorString ? g_rccl.GetErrorString(r) : "?")); }
  e->nranks = nranks;
  return 0;
}
int mpcq_comm_share(mpcq_engine* e, mpcq_engine* owner) {
  ENTER(e);
  if (!owner || owner == e) return fail(MPCQ_ERR_INVALID, "mpcq_comm_share: bad owner");
  if (e->comm) return fail(MPCQ_ERR_STATE, "communicator already initialised");
  if (!owner->comm || owner->comm_borrowed) return fail(MPCQ_ERR_STATE, "mpcq_comm_share: the owner has no communicator of its own");
  if (owner->cfg.device != e->cfg.device) return fail(MPCQ_ERR_INVALID, "mpcq_comm_share: the two engines live on different devices");
  e->comm = owner->comm;
  e->comm_borrowed = true;
  e->nranks = owner->nranks;
  return 0;
}
int mpcq_allreduce_tracking_stats(mpcq_engine* e, double out[5]) {
  ENTER(e);
  int rc = e->stats(nullptr);  // local 5-vector on the device
  if (rc) return rc;
  if (e->comm) {
    // slots 0,1,2,4 sum; slot 3 max: reduce [s0,s1,s2,0,s4] with SUM into d[0..4], [s3] with MAX into d[5]
    double* d = e->d_stats5;
    HIP_TRY(hipMemcpyAsync(d + 5, d + 3, sizeof(double), hipMemcpyDeviceToDevice, e->stream));
    HIP_TRY(hipMemsetAsync(d + 3, 0, sizeof(double), e->stream));
    int r = g_rccl.AllReduce(d, d, 5, NCCL_FLOAT64, NCCL_SUM, e->comm, e->stream);
    if (!r) r = g_rccl.AllReduce(d + 5, d + 5, 1, NCCL_FLOAT64, NCCL_MAX, e->comm, e->stream);
    if (r) return fail(MPCQ_ERR_COMM, std::string("ncclAllReduce: ") + (g_rccl.GetErrorString ? g_rccl.GetErrorString(r) : "?"));
    HIP_TRY(hipMemcpyAsync(d + 3, d + 5, sizeof(double), hipMemcpyDeviceToDevice, e->stream));
  }
  HIP_TRY(hipMemcpyAsync(out, e->d_stats5, 5 * sizeof(double), hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  return 0;
}
int mpcq_get_state(mpcq_engine* e, double* X, double* U, double* mu, double* C, double* xpp, int32_t* hp, int32_t* idx) { ENTER(e); return e->get_state(X, U, mu, C, xpp, hp, idx); }
int mpcq_set_state(mpcq_engine* e, const double* X, const double* U, const double* mu, const double* C, const double* xpp, const int32_t* hp, const int32_t* idx) { ENTER(e); return e->set_state(X, U, mu, C, xpp, hp, idx); }
int mpcq_get_solver_state(mpcq_engine* e, int32_t* qp_iter, double* stats4, int32_t* finished) { ENTER(e); return e->get_solver_state(qp_iter, stats4, finished); }
int mpcq_set_solver_state(mpcq_engine* e, const int32_t* qp_iter, const double* stats4, const int32_t* finished) { ENTER(e); return e->set_solver_state(qp_iter, stats4, finished); }

// ---- continuous operation: trajectory slots (mpcq_replan.hpp)
namespace {
// The argument rules of what plans flights: mpcq_replan and mpcq_replan_nonlinear (through replan_inputs), mpcq_mission_set and
// mpcq_mission_set_legs (`who`), in the order a caller meets them.  The rules of a queue (L, nonlinear, its size) apply with `queue` only.
struct PlanArgs {
  bool has_wp; int n_wp;               // n_wp is checked when there are waypoints
  bool limits_ok; const char* limits;  // the caller's own check of v_max, a_max and dt, and its rule in words
  int derivative;
  bool opts_ok;                        // the caller's own check of its options
  bool queue = false, L_first = false;
  int L = 0, nonlinear = 0;
  size_t B = 0;
};
int plan_checks(const std::string& who, const PlanArgs& a) {
  const bool bad_n_wp = a.has_wp && (a.n_wp < 1 || a.n_wp > mpcq::replan::MAXV - 1), bad_L = a.queue && a.L < 1;
  // (the one place the callers' orders differ: mpcq_mission_set_legs, where waypoints are optional, has looked at L before n_wp since it
  //  exists; mpcq_mission_set looks at n_wp first, as the replan calls it grew out of do.  Kept: callers see the message.)
  if (a.L_first && bad_L) return fail(MPCQ_ERR_INVALID, who + ": L must be >= 1");
  if (bad_n_wp) return fail(MPCQ_ERR_INVALID, who + ": n_wp outside 1..7");
  if (bad_L) return fail(MPCQ_ERR_INVALID, who + ": L must be >= 1");
  if (a.queue && a.nonlinear != 0 && a.nonlinear != 1) return fail(MPCQ_ERR_INVALID, who + ": nonlinear must be 0 or 1");
  if (!a.limits_ok) return fail(MPCQ_ERR_INVALID, who + ": " + a.limits);
  if (a.derivative < 2 || a.derivative > 4) return fail(MPCQ_ERR_INVALID, who + ": derivative_to_optimize outside 2..4");
  if (!a.opts_ok) return fail(MPCQ_ERR_INVALID, who + ": options out of range");
  if (a.queue && a.B * (size_t)a.L > 0x7fffffffull) return fail(MPCQ_ERR_INVALID, who + ": queue too large (B x L x n_wp)");
  return 0;
}
// What the three replan entry points (`who`) share behind their argument checks: the state checks, in the order a caller meets them, and
// the staging on the device -- start points, mask and result codes.  The caller's own inputs (`head` doubles: waypoints, or radius and
// v_max) go to in.head, which it fills itself.
struct ReplanInputs {
  EngineView t;
  double* head;               // [head] the caller's inputs
  const double* start;        // start points [B,start_stride]: the caller's [B,3] or the plant state
  int start_stride;
  const int* mask;            // nullptr: the quadrotors whose finished flag is set
  int* code;                  // [B] result codes
  double* extra;              // `extra` doubles of staging behind the inputs
};
int replan_stage(const std::string& who, mpcq_engine* e, const double* start, const int32_t* mask, size_t head, size_t extra, ReplanInputs& in) {
  if (const int rc = needs_trajectories(e, who)) return rc;
  if (!start && !e->have_sim) return fail(MPCQ_ERR_STATE, who + " without start points needs mpcq_sim_reset first (the plant state)");
  in.t = e->view();
  const size_t B = e->B;
  HIP_TRY(e->rp.d_in.grow(head + B * 3 + extra));
  HIP_TRY(e->rp.d_int.grow(ReplanStaging::n_ints(B)));
  double* d_in = e->rp.d_in.p;
  const ReplanStaging::Ints d = e->rp.ints(B);
  if (start) HIP_TRY(hipMemcpyAsync(d_in + head, start, B * 3 * sizeof(double), hipMemcpyHostToDevice, e->stream));
  if (mask) HIP_TRY(hipMemcpyAsync(d.mask, mask, B * sizeof(int), hipMemcpyHostToDevice, e->stream));
  in.head = d_in;
  in.start = start ? d_in + head : in.t.plant;
  in.start_stride = start ? 3 : 13;
  in.mask = mask ? d.mask : nullptr;
  in.code = d.code;
  in.extra = d_in + head + B * 3;
  return 0;
}
// mpcq_replan and mpcq_replan_nonlinear: the checks, the staging and the waypoints [B,n_wp,3] at in.head
int replan_inputs(const char* who_, mpcq_engine* e, const double* start, const double* wp, int32_t n_wp, bool limits_ok, const char* limits,
                  int32_t derivative_to_optimize, bool opts_ok, const int32_t* mask, size_t extra, ReplanInputs& in) {
  const std::string who(who_);
  if (!wp) return fail(MPCQ_ERR_INVALID, who + ": null waypoints");
  PlanArgs a{true, n_wp, limits_ok, limits, derivative_to_optimize, opts_ok};
  if (const int rc = plan_checks(who, a)) return rc;
  const size_t nwp = (size_t)e->B * n_wp * 3;
  if (const int rc = replan_stage(who, e, start, mask, nwp, extra, in)) return rc;
  HIP_TRY(hipMemcpyAsync(in.head, wp, nwp * sizeof(double), hipMemcpyHostToDevice, e->stream));
  return 0;
}
}  // namespace

int mpcq_replan(mpcq_engine* e, const double* start, const double* wp, int32_t n_wp, double v_max, double a_max, int32_t derivative_to_optimize,
                double dt, const int32_t* mask, int32_t* out) {
  ENTER(e);
  ReplanInputs in;
  if (const int rc = replan_inputs("mpcq_replan", e, start, wp, n_wp, v_max > 0 && a_max > 0 && dt > 0, "v_max, a_max and dt must be > 0", derivative_to_optimize, true, mask, 0, in)) return rc;
  hipLaunchKernelGGL(mpcq::replan::replan_kernel, dim3(e->B), dim3(64), sizeof(mpcq::replan::Lds), e->stream, in.t.traj, in.t.Tmax, in.t.len, in.t.idx, in.t.finished,
                     in.start, in.start_stride, (const double*)in.head, (int)n_wp, v_max, a_max, (int)derivative_to_optimize, dt, in.mask, in.code);
  HIP_TRY(hipGetLastError());
  if (out) HIP_TRY(hipMemcpyAsync(out, in.code, (size_t)e->B * sizeof(int), hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  return 0;
}

int mpcq_replan_nonlinear(mpcq_engine* e, const double* start, const double* wp, int32_t n_wp, double v_max, double a_max, int32_t derivative_to_optimize,
                          double dt, const int32_t* mask, int32_t* out, const mpcq_minsnap_nl_options* opts, double* info, double* pieces, double* d_free) {
  ENTER(e);
  const mpcq_nl::Opts o = mpcq_nl::nl_opts_from(opts);   // (NULL: MPCQ_MINSNAP_NL_DEFAULTS)
  const size_t B = e->B, n_info = B * 6, n_pc = B * n_wp * 33, n_df = B * (n_wp - 1) * 9;   // (used behind the check of n_wp only)
  ReplanInputs in;
  if (const int rc = replan_inputs("mpcq_replan_nonlinear", e, start, wp, n_wp, v_max > 0 && a_max > 0 && dt > 0 && std::isfinite(v_max) && std::isfinite(a_max),
                                   "v_max, a_max and dt must be finite and > 0", derivative_to_optimize, mpcq_nl::nl_opts_valid(o), mask, n_info + n_pc + n_df, in))
    return rc;
  double* d_info = in.extra;
  double* d_pc = d_info + n_info;
  double* d_df = d_pc + n_pc;
  hipLaunchKernelGGL(mpcq::replan::replan_nl_kernel, dim3(e->B), dim3(64), sizeof(mpcq::replan::NlLds), e->stream, in.t.traj, in.t.Tmax, in.t.len, in.t.idx,
                     in.t.finished, in.start, in.start_stride, (const double*)in.head, (int)n_wp, v_max, a_max, (int)derivative_to_optimize, dt, in.mask, in.code, o,
                     info ? d_info : nullptr, pieces ? d_pc : nullptr, d_free && n_df ? d_df : nullptr);
  HIP_TRY(hipGetLastError());
  if (out) HIP_TRY(hipMemcpyAsync(out, in.code, B * sizeof(int), hipMemcpyDeviceToHost, e->stream));
  if (info) HIP_TRY(hipMemcpyAsync(info, d_info, n_info * sizeof(double), hipMemcpyDeviceToHost, e->stream));
  if (pieces) HIP_TRY(hipMemcpyAsync(pieces, d_pc, n_pc * sizeof(double), hipMemcpyDeviceToHost, e->stream));
  if (d_free && n_df) HIP_TRY(hipMemcpyAsync(d_free, d_df, n_df * sizeof(double), hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  return 0;
}

// The reference's 'circle' request (mpcq_circle.hpp): closed-form circle flights generated on the device.
int mpcq_replan_circle(mpcq_engine* e, const double* start, const double* radius, const double* v_max, int32_t kind, double dt, double t_max,
                       const int32_t* mask, int32_t* out) {
  ENTER(e);
  const std::string who("mpcq_replan_circle");
  if (!radius || !v_max) return fail(MPCQ_ERR_INVALID, who + ": null radius or v_max");
  if (kind != MPCQ_CIRCLE_ACC_DEC && kind != MPCQ_CIRCLE_CONSTANT && kind != MPCQ_CIRCLE_ACCELERATING) return fail(MPCQ_ERR_INVALID, who + ": unknown kind");
  if (!(dt > 0 && std::isfinite(dt))) return fail(MPCQ_ERR_INVALID, who + ": dt must be finite and > 0");
  if (kind == MPCQ_CIRCLE_ACCELERATING && !(t_max > 0 && std::isfinite(t_max))) return fail(MPCQ_ERR_INVALID, who + ": t_max must be finite and > 0");
  const size_t B = e->B;
  ReplanInputs in;
  if (const int rc = replan_stage(who, e, start, mask, 2 * B, 0, in)) return rc;   // head: radius [B] | v_max [B]
  HIP_TRY(hipMemcpyAsync(in.head, radius, B * sizeof(double), hipMemcpyHostToDevice, e->stream));
  HIP_TRY(hipMemcpyAsync(in.head + B, v_max, B * sizeof(double), hipMemcpyHostToDevice, e->stream));
  hipLaunchKernelGGL(mpcq::replan::circle_kernel, dim3(e->B), dim3(64), sizeof(mpcq::replan::Lds), e->stream, in.t.traj, in.t.Tmax, in.t.len, in.t.idx, in.t.finished,
                     in.start, in.start_stride, (const double*)in.head, (const double*)(in.head + B), (int)kind, dt, t_max, in.mask, in.code);
  HIP_TRY(hipGetLastError());
  if (out) HIP_TRY(hipMemcpyAsync(out, in.code, B * sizeof(int), hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  return 0;
}

int mpcq_replace_trajectories(mpcq_engine* e, const int32_t* idx, int32_t count, const double* traj, const int32_t* len) {
  ENTER(e);
  if (!idx || !traj || !len) return fail(MPCQ_ERR_INVALID, "mpcq_replace_trajectories: null argument");
  if (const int rc = needs_trajectories(e, "mpcq_replace_trajectories")) return rc;
  const EngineView t = e->view();
  if (count < 0 || count > e->B) return fail(MPCQ_ERR_INVALID, "mpcq_replace_trajectories: count outside 0..B");
  std::vector<char> seen(e->B, 0);
  for (int j = 0; j < count; ++j) {
    if (idx[j] < 0 || idx[j] >= e->B) return fail(MPCQ_ERR_INVALID, "mpcq_replace_trajectories: index out of range");
    if (seen[idx[j]]++) return fail(MPCQ_ERR_INVALID, "mpcq_replace_trajectories: duplicate index");
    if (len[j] < 1 || len[j] > t.Tmax) return fail(MPCQ_ERR_INVALID, "trajectory length out of range");
  }
  if (count == 0) return 0;
  const size_t rows = (size_t)count * t.Tmax * 13;
  HIP_TRY(e->rp.d_in.grow(rows));
  HIP_TRY(e->rp.d_int.grow(ReplanStaging::n_ints(e->B)));
  double* d_rows = e->rp.d_in.p;
  int *d_idx = e->rp.ints(e->B).idx, *d_len = e->rp.ints(e->B).len;
  HIP_TRY(hipMemcpyAsync(d_rows, traj, rows * sizeof(double), hipMemcpyHostToDevice, e->stream));
  HIP_TRY(hipMemcpyAsync(d_idx, idx, (size_t)count * sizeof(int), hipMemcpyHostToDevice, e->stream));
  HIP_TRY(hipMemcpyAsync(d_len, len, (size_t)count * sizeof(int), hipMemcpyHostToDevice, e->stream));
  hipLaunchKernelGGL(mpcq::replan::install_kernel, dim3(count), dim3(64), sizeof(mpcq::replan::Lds), e->stream, t.traj, t.Tmax, t.len, t.idx, t.finished,
                     (const double*)d_rows, (const int*)d_idx, (const int*)d_len);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(e->stream));
  return 0;
}

// ---- device missions (mpcq_mission.hpp; state, layout and launch: Mission, mission_launch)
namespace {
// What mpcq_mission_set and mpcq_mission_set_legs (`who`) end in, behind their argument checks: the queue, the legs table, the leg counters
// and an empty log on the device, the mission on.  wp may be NULL (no waypoint leg; n_wp is 0 then).
int mission_begin(const std::string& who, mpcq_engine* e, const mpcq_leg* legs, const double* wp, int32_t L, int32_t n_wp, int32_t order, double dt,
                  int32_t nonlinear, const mpcq_nl::Opts& o, const int32_t* leg0) {
  const size_t B = e->B, nl = B * (size_t)L;
  if (nl * (n_wp > 0 ? n_wp : 1) * 3 > 0x7fffffffull) return fail(MPCQ_ERR_INVALID, who + ": queue too large (B x L x n_wp)");
  if (leg0)
    for (size_t b = 0; b < B; ++b)
      if (leg0[b] < 0 || leg0[b] > L) return fail(MPCQ_ERR_INVALID, who + ": leg0 outside 0..L");
  if (const int rc = needs_trajectories(e, who)) return rc;
  HIP_TRY(hipStreamSynchronize(e->stream));   // (launches of an mpcq_step_device_async may still read the queue that is replaced)
  Mission& ms = e->ms;
  ms.on = false;
  e->end_exploration();
  if (wp) HIP_TRY(ms.d_wp.grow(nl * n_wp * 3));
  else ms.d_wp.release();
  HIP_TRY(ms.d_legs.grow(nl));
  HIP_TRY(ms.d_int.grow(Mission::n_ints(B, nl)));
  if (nonlinear) HIP_TRY(ms.d_info.grow(B * 6));
  std::vector<int> h(Mission::n_ints(B, nl), 0);   // the start values: no flight installed, no leg consumed
  const Mission::Ints hi = Mission::ints_at(h.data(), B, nl);
  for (size_t b = 0; b < B; ++b) { hi.leg[b] = leg0 ? leg0[b] : 0; hi.last_code[b] = MPCQ_REPLAN_SKIPPED; }
  for (size_t k = 0; k < nl; ++k) { hi.leg_code[k] = MPCQ_REPLAN_SKIPPED; hi.leg_period[k] = -1; }
  if (wp) HIP_TRY(hipMemcpyAsync(ms.d_wp.p, wp, nl * n_wp * 3 * sizeof(double), hipMemcpyHostToDevice, e->stream));
  HIP_TRY(hipMemcpyAsync(ms.d_legs.p, legs, nl * sizeof(mpcq_leg), hipMemcpyHostToDevice, e->stream));
  HIP_TRY(hipMemcpyAsync(ms.d_int.p, h.data(), h.size() * sizeof(int), hipMemcpyHostToDevice, e->stream));
  const std::vector<double> nan(nonlinear ? B * 6 : 0, std::nan(""));   // (info: NaN rows until a flight is installed)
  if (nonlinear) HIP_TRY(hipMemcpyAsync(ms.d_info.p, nan.data(), nan.size() * sizeof(double), hipMemcpyHostToDevice, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  ms.L = L; ms.n_wp = wp ? n_wp : 0; ms.order = order; ms.nonlinear = nonlinear;
  ms.dt = dt; ms.opts = o;
  ms.periods = 0;
  ms.on = true;
  return 0;
}
}  // namespace

int mpcq_mission_set(mpcq_engine* e, const double* wp, int32_t L, int32_t n_wp, double v_max, double a_max, int32_t derivative_to_optimize, double dt,
                     int32_t nonlinear, const mpcq_minsnap_nl_options* opts, const int32_t* leg0) {
  ENTER(e);
  const std::string who("mpcq_mission_set");
  if (!wp) return fail(MPCQ_ERR_INVALID, who + ": null waypoints");
  const mpcq_nl::Opts o = mpcq_nl::nl_opts_from(opts);   // (NULL: MPCQ_MINSNAP_NL_DEFAULTS)
  PlanArgs a{true, n_wp, v_max > 0 && a_max > 0 && dt > 0 && std::isfinite(v_max) && std::isfinite(a_max) && std::isfinite(dt),
             "v_max, a_max and dt must be finite and > 0", derivative_to_optimize, !nonlinear || mpcq_nl::nl_opts_valid(o)};
  a.queue = true; a.L = L; a.nonlinear = nonlinear; a.B = e->B;
  if (const int rc = plan_checks(who, a)) return rc;
  // the special case of mpcq_mission_set_legs: every leg a waypoint leg with the call's limits
  mpcq_leg one;
  one.kind = MPCQ_LEG_WAYPOINTS; one.reserved = 0; one.v_max = v_max; one.a_max = a_max; one.radius = 0.0;
  const std::vector<mpcq_leg> legs((size_t)e->B * (size_t)L, one);
  return mission_begin(who, e, legs.data(), wp, L, n_wp, derivative_to_optimize, dt, nonlinear, o, leg0);
}
int mpcq_mission_set_legs(mpcq_engine* e, const mpcq_leg* legs, const double* wp, int32_t L, int32_t n_wp, int32_t derivative_to_optimize, double dt,
                          int32_t nonlinear, const mpcq_minsnap_nl_options* opts, const int32_t* leg0) {
  ENTER(e);
  const std::string who("mpcq_mission_set_legs");
  if (!legs) return fail(MPCQ_ERR_INVALID, who + ": null legs");
  const mpcq_nl::Opts o = mpcq_nl::nl_opts_from(opts);   // (NULL: MPCQ_MINSNAP_NL_DEFAULTS)
  PlanArgs a{wp != nullptr, n_wp, dt > 0 && std::isfinite(dt), "dt must be finite and > 0", derivative_to_optimize, !nonlinear || mpcq_nl::nl_opts_valid(o)};
  a.queue = true; a.L_first = true; a.L = L; a.nonlinear = nonlinear; a.B = e->B;
  if (const int rc = plan_checks(who, a)) return rc;
  auto positive = [](double x) { return x > 0 && std::isfinite(x); };
  for (size_t k = 0, nl = (size_t)e->B * (size_t)L; k < nl; ++k) {
    const mpcq_leg& lg = legs[k];
    if (lg.kind != MPCQ_LEG_WAYPOINTS && lg.kind != MPCQ_LEG_CIRCLE) return fail(MPCQ_ERR_INVALID, who + ": unknown leg kind");
    if (lg.reserved != 0) return fail(MPCQ_ERR_INVALID, who + ": reserved must be 0");
    if (lg.kind == MPCQ_LEG_WAYPOINTS && !wp) return fail(MPCQ_ERR_INVALID, who + ": a waypoint leg needs waypoints");
    if (!positive(lg.v_max) || !positive(lg.a_max) || (lg.kind == MPCQ_LEG_CIRCLE && !positive(lg.radius)))
      return fail(MPCQ_ERR_INVALID, who + ": v_max, a_max and (circle legs) radius of every leg must be finite and > 0");
  }
  return mission_begin(who, e, legs, wp, L, wp ? n_wp : 0, derivative_to_optimize, dt, nonlinear, o, leg0);   // (n_wp is not read without wp)
}
int mpcq_mission_get(mpcq_engine* e, int32_t* leg, int32_t* installed, int32_t* last_code, int32_t* leg_code, int32_t* leg_period, double* info) {
  ENTER(e);
  const Mission& ms = e->ms;
  if (!ms.on) return fail(MPCQ_ERR_STATE, "mpcq_mission_get: no mission set");
  const size_t B = e->B, nl = B * (size_t)ms.L;
  const Mission::Ints d = ms.ints(B);
  if (leg) HIP_TRY(hipMemcpyAsync(leg, d.leg, B * sizeof(int), hipMemcpyDeviceToHost, e->stream));
  if (installed) HIP_TRY(hipMemcpyAsync(installed, d.installed, B * sizeof(int), hipMemcpyDeviceToHost, e->stream));
  if (last_code) HIP_TRY(hipMemcpyAsync(last_code, d.last_code, B * sizeof(int), hipMemcpyDeviceToHost, e->stream));
  if (leg_code) HIP_TRY(hipMemcpyAsync(leg_code, d.leg_code, nl * sizeof(int), hipMemcpyDeviceToHost, e->stream));
  if (leg_period) HIP_TRY(hipMemcpyAsync(leg_period, d.leg_period, nl * sizeof(int), hipMemcpyDeviceToHost, e->stream));
  if (info && ms.nonlinear) HIP_TRY(hipMemcpyAsync(info, ms.d_info.p, B * 6 * sizeof(double), hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  if (info && !ms.nonlinear)
    for (size_t k = 0; k < B * 6; ++k) info[k] = std::nan("");
  return 0;
}
int mpcq_mission_stop(mpcq_engine* e) {
  ENTER(e);
  if (const int rc = feature_stop(e, e->ms, "mpcq_mission_stop: no mission set")) return rc;
  e->end_exploration();
  return 0;
}

// ---- exploration (mpcq_explore.hpp; state, layout and launch: Explore, explore_launch)
int mpcq_explore_start(mpcq_engine* e, const mpcq_explore_rule* rules, uint64_t rule_size, const uint8_t* leg_mask, const double* env0, const int64_t* samples0) {
  ENTER(e);
  const std::string who("mpcq_explore_start");
  if (!e->ms.on) return fail(MPCQ_ERR_STATE, who + ": no mission set (the limits go into its legs table)");
  if (!rules) return fail(MPCQ_ERR_INVALID, who + ": rules is NULL");
  if (rule_size != sizeof(mpcq_explore_rule))
    return fail(MPCQ_ERR_INVALID, who + ": rule_size " + std::to_string(rule_size) + " is not this library's sizeof(mpcq_explore_rule) = " + std::to_string(sizeof(mpcq_explore_rule)));
  if (!env0 != !samples0) return fail(MPCQ_ERR_INVALID, who + ": env0 and samples0 come together (a checkpoint), or both NULL");
  const size_t B = e->B, nl = B * (size_t)e->ms.L;
  // every rule is checked before anything of the engine changes
  for (size_t b = 0; b < B; ++b) {
    const mpcq_explore_rule& r = rules[b];
    auto bad = [&](const char* field, const char* rule) { return fail(MPCQ_ERR_INVALID, who + ": quadrotor " + std::to_string(b) + ": " + field + " " + rule); };
    const struct { const char* name; double v; } fields[] = {{"step", r.step}, {"desired", r.desired}, {"v_limit", r.v_limit}, {"a_limit", r.a_limit}};
    for (const auto& f : fields)
      if (!(std::isfinite(f.v) && f.v > 0)) return bad(f.name, "must be finite and > 0");
    if (r.mode != MPCQ_EXPLORE_LAST_FLIGHT && r.mode != MPCQ_EXPLORE_CUMULATIVE) return bad("mode", "must be 0 (last flight) or 1 (cumulative)");
    if (r.axes < 1 || r.axes > 7) return bad("axes", "must be in 1..7");
    if (samples0 && samples0[b] < 0) return bad("samples0", "must be >= 0");
  }
  // The new state goes to buffers of its own and takes the old one's place only once it is complete on the device: a failed allocation or
  // copy leaves the engine exploring as it did (or not at all).
  Explore fresh;
  const std::string no_mem = who + ": cannot allocate the rules, the envelopes and the log";
  if (grow_or_fail(fresh.d_rules, B, no_mem) || grow_or_fail(fresh.d_mask, nl, no_mem) || grow_or_fail(fresh.d_f64, Explore::n_f64(B, nl), no_mem) ||
      grow_or_fail(fresh.d_samples, B, no_mem))
    return MPCQ_ERR_DEVICE;
  std::vector<double> f64(Explore::n_f64(B, nl), std::nan(""));   // (leg_limits NaN: not written)
  const Explore::F64 hf = Explore::f64_at(f64.data(), B);
  std::vector<int64_t> smp(B, 0);
  for (size_t b = 0; b < B; ++b) {
    const bool have = samples0 && samples0[b] > 0;   // (samples == 0 reads as min = max = 0)
    for (int k = 0; k < 6; ++k) hf.env[b * 6 + k] = have ? env0[b * 6 + k] : 0.0;
    if (have) smp[b] = samples0[b];
  }
  const std::vector<unsigned char> all(leg_mask ? 0 : nl, 1);
  HIP_TRY(hipStreamSynchronize(e->stream));   // (launches of an mpcq_step_device_async may still use the state that is replaced)
  HIP_TRY(hipMemcpyAsync(fresh.d_rules.p, rules, B * sizeof(mpcq_explore_rule), hipMemcpyHostToDevice, e->stream));
  HIP_TRY(hipMemcpyAsync(fresh.d_mask.p, leg_mask ? leg_mask : all.data(), nl, hipMemcpyHostToDevice, e->stream));
  HIP_TRY(hipMemcpyAsync(fresh.d_f64.p, f64.data(), f64.size() * sizeof(double), hipMemcpyHostToDevice, e->stream));
  HIP_TRY(hipMemcpyAsync(fresh.d_samples.p, smp.data(), B * sizeof(int64_t), hipMemcpyHostToDevice, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  e->ex = std::move(fresh);
  e->ex.on = true;
  return 0;
}
int mpcq_explore_get(mpcq_engine* e, double* env, int64_t* samples, double* leg_limits) {
  ENTER(e);
  const Explore& ex = e->ex;
  if (!ex.on) return fail(MPCQ_ERR_STATE, "mpcq_explore_get: no exploration running");
  const size_t B = e->B, nl = B * (size_t)e->ms.L;
  const Explore::F64 d = ex.f64(B);
  if (env) HIP_TRY(hipMemcpyAsync(env, d.env, B * 6 * sizeof(double), hipMemcpyDeviceToHost, e->stream));
  if (leg_limits) HIP_TRY(hipMemcpyAsync(leg_limits, d.leg_limits, nl * 3 * sizeof(double), hipMemcpyDeviceToHost, e->stream));
  if (samples) HIP_TRY(hipMemcpyAsync(samples, ex.d_samples.p, B * sizeof(int64_t), hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  return 0;
}
int mpcq_explore_stop(mpcq_engine* e) { ENTER(e); return feature_stop(e, e->ex, "mpcq_explore_stop: no exploration running"); }

// ---- flight recorder (mpcq_record.hpp; state: Recorder; the launches: EngineT::rec_snapshot / rec_write)
#define MPCQ_RECORD_ALL 511
int mpcq_record_start(mpcq_engine* e, const int32_t* quads, int32_t count, int32_t fields, int32_t every, int32_t capacity) {
  ENTER(e);
  Recorder& r = e->rec;
  if (r.on) return fail(MPCQ_ERR_STATE, "mpcq_record_start: a recording is active (mpcq_record_stop first)");
  if (quads && count <= 0) return fail(MPCQ_ERR_INVALID, "mpcq_record_start: count must be > 0");
  if (fields == 0 || (fields & ~MPCQ_RECORD_ALL)) return fail(MPCQ_ERR_INVALID, "mpcq_record_start: fields empty or unknown bits");
  if (every < 1 || capacity < 1) return fail(MPCQ_ERR_INVALID, "mpcq_record_start: every and capacity must be >= 1");
  if (!e->nb && (fields & (MPCQ_RECORD_RGP_MU | MPCQ_RECORD_RGP_C))) return fail(MPCQ_ERR_INVALID, "mpcq_record_start: RGP fields on an engine with nb = 0");
  const int n = quads ? count : e->B;
  std::vector<int> sel(n);
  std::vector<char> seen(e->B, 0);
  for (int j = 0; j < n; ++j) {
    sel[j] = quads ? quads[j] : j;
    if (sel[j] < 0 || sel[j] >= e->B) return fail(MPCQ_ERR_INVALID, "mpcq_record_start: quadrotor index out of range");
    if (seen[sel[j]]++) return fail(MPCQ_ERR_INVALID, "mpcq_record_start: duplicate quadrotor index");
  }
  Recorder nr;
  nr.fields = fields; nr.every = every; nr.capacity = capacity; nr.count = n;
  nr.sorted = sel;
  std::sort(nr.sorted.begin(), nr.sorted.end());
  nr.pos.resize(n);
  for (int j = 0; j < n; ++j) nr.pos[j] = (int)(std::lower_bound(nr.sorted.begin(), nr.sorted.end(), sel[j]) - nr.sorted.begin());
  for (const Group& g : e->groups) {   // the part of the selection inside every group of mpcq_sim_steps, and inside the whole batch
    nr.glo.push_back((int)(std::lower_bound(nr.sorted.begin(), nr.sorted.end(), g.b0) - nr.sorted.begin()));
    nr.ghi.push_back((int)(std::lower_bound(nr.sorted.begin(), nr.sorted.end(), g.b0 + g.n) - nr.sorted.begin()));
  }
  // (a return from here on releases what `nr` holds by then; the engine's recorder is touched by the last statement only)
  auto need = [](auto& buf, size_t elems, const char* what) {
    return grow_or_fail(buf, elems, "mpcq_record_start: cannot allocate " + std::to_string(elems * sizeof(*buf.p)) + " bytes for " + what);
  };
  int rc = need(nr.d_sel, (size_t)n, "the selection");
  for (int f = 0; f < mpcq::record::NF && !rc; ++f) {
    if (!(fields >> f & 1)) continue;
    const size_t elems = (size_t)capacity * n * mpcq::record::width(f, e->nb);
    rc = f == mpcq::record::F_SOLVER ? need(nr.d_solver, elems, "the solver field") : need(nr.d_f[f], elems, "a recorded field");
  }
  if (!rc && (fields & MPCQ_RECORD_DRAG)) rc = need(nr.d_snap, (size_t)n * mpcq::record::SNAP, "the drag snapshot");
  if (rc) return rc;
  if (hipMemcpyAsync(nr.d_sel.p, nr.sorted.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice, e->stream) != hipSuccess)
    return fail(MPCQ_ERR_DEVICE, "mpcq_record_start: copy of the selection failed");
  if (hipStreamSynchronize(e->stream) != hipSuccess) return fail(MPCQ_ERR_DEVICE, "mpcq_record_start: hipStreamSynchronize failed");
  nr.period_of.reserve(capacity < (1 << 20) ? capacity : (1 << 20));
  nr.on = true;
  r = std::move(nr);
  return 0;
}
int mpcq_record_info(mpcq_engine* e, int32_t* rows, int64_t* dropped, int64_t* periods) {
  ENTER(e);
  const Recorder& r = e->rec;
  if (!r.on) return fail(MPCQ_ERR_STATE, "mpcq_record_info: no active recording");
  if (rows) *rows = r.rows;
  if (dropped) *dropped = r.dropped;
  if (periods) *periods = r.periods;
  return 0;
}
int mpcq_record_get(mpcq_engine* e, int32_t field, double* out) {
  ENTER(e);
  const Recorder& r = e->rec;
  if (!r.on) return fail(MPCQ_ERR_STATE, "mpcq_record_get: no active recording");
  if (field <= 0 || (field & (field - 1)) || !(field & r.fields) || field == MPCQ_RECORD_SOLVER)
    return fail(MPCQ_ERR_INVALID, "mpcq_record_get: field is not one recorded double field (MPCQ_RECORD_SOLVER: mpcq_record_get_solver)");
  if (!out) return fail(MPCQ_ERR_INVALID, "null argument");
  int f = 0;
  while (!(field >> f & 1)) ++f;
  return rec_read(e, (const double*)r.d_f[f].p, mpcq::record::width(f, e->nb), out);
}
int mpcq_record_get_solver(mpcq_engine* e, int32_t* out) {
  ENTER(e);
  const Recorder& r = e->rec;
  if (!r.on) return fail(MPCQ_ERR_STATE, "mpcq_record_get_solver: no active recording");
  if (!(r.fields & MPCQ_RECORD_SOLVER)) return fail(MPCQ_ERR_INVALID, "mpcq_record_get_solver: MPCQ_RECORD_SOLVER was not recorded");
  if (!out) return fail(MPCQ_ERR_INVALID, "null argument");
  return rec_read(e, (const int*)r.d_solver.p, 4, (int*)out);
}
int mpcq_record_get_periods(mpcq_engine* e, int64_t* out) {
  ENTER(e);
  const Recorder& r = e->rec;
  if (!r.on) return fail(MPCQ_ERR_STATE, "mpcq_record_get_periods: no active recording");
  if (!out) return fail(MPCQ_ERR_INVALID, "null argument");
  for (int k = 0; k < r.rows; ++k) out[k] = r.period_of[k];
  return 0;
}
int mpcq_record_clear(mpcq_engine* e) {
  ENTER(e);
  Recorder& r = e->rec;
  if (!r.on) return fail(MPCQ_ERR_STATE, "mpcq_record_clear: no active recording");
  r.rows = 0; r.dropped = 0; r.period_of.clear();
  return 0;
}
int mpcq_record_stop(mpcq_engine* e) { ENTER(e); return feature_stop(e, e->rec, "mpcq_record_stop: no active recording"); }

// ---- incident recorder (mpcq_blackbox.hpp; state: BlackBox; the launches: EngineT::bb_snapshot / bb_write)
int mpcq_blackbox_start(mpcq_engine* e, const int32_t* quads, int32_t count, int32_t fields, int32_t pre, int32_t post, const mpcq_blackbox_rule* rules) {
  ENTER(e);
  namespace bx = mpcq::blackbox;
  const std::string who("mpcq_blackbox_start");
  if (e->bb.on) return fail(MPCQ_ERR_STATE, who + ": a black box is running (mpcq_blackbox_stop first)");
  if (quads && count <= 0) return fail(MPCQ_ERR_INVALID, who + ": count must be > 0");
  if (fields == 0 || (fields & ~MPCQ_RECORD_ALL)) return fail(MPCQ_ERR_INVALID, who + ": fields empty or unknown bits");
  if (!e->nb && (fields & (MPCQ_RECORD_RGP_MU | MPCQ_RECORD_RGP_C))) return fail(MPCQ_ERR_INVALID, who + ": RGP fields on an engine with nb = 0");
  if (pre < 0 || post < 0) return fail(MPCQ_ERR_INVALID, who + ": pre and post must be >= 0");
  if ((long long)pre + 1 + post > 65536) return fail(MPCQ_ERR_INVALID, who + ": ring depth pre + 1 + post must be <= 65536");
  if (!rules) return fail(MPCQ_ERR_INVALID, who + ": rules is NULL");
  const int n = quads ? count : e->B;
  std::vector<int> sel(n);
  std::vector<char> seen(e->B, 0);
  for (int j = 0; j < n; ++j) {
    sel[j] = quads ? quads[j] : j;
    if (sel[j] < 0 || sel[j] >= e->B) return fail(MPCQ_ERR_INVALID, who + ": quadrotor index out of range");
    if (seen[sel[j]]++) return fail(MPCQ_ERR_INVALID, who + ": duplicate quadrotor index");
  }
  // every rule is checked before anything is allocated
  for (int j = 0; j < n; ++j) {
    const mpcq_blackbox_rule& r = rules[j];
    auto bad = [&](const char* field, const char* rule) { return fail(MPCQ_ERR_INVALID, who + ": quadrotor " + std::to_string(sel[j]) + ": " + field + " " + rule); };
    if (r.causes & ~bx::C_ALL) return bad("causes", "has unknown bits");
    const struct { const char* name; double v; int cause; } th[] = {{"err_pos", r.err_pos, MPCQ_BB_ERR_POS}, {"speed", r.speed, MPCQ_BB_SPEED},
                                                                    {"tilt_cos", r.tilt_cos, MPCQ_BB_TILT}, {"cost", r.cost, MPCQ_BB_COST}};
    for (const auto& t : th)
      if ((r.causes & t.cause) && std::isnan(t.v)) return bad(t.name, "is NaN and its cause is enabled");
    if (r.err_pos < 0) return bad("err_pos", "must be >= 0");
    if (r.speed < 0) return bad("speed", "must be >= 0");
  }
  BlackBox nr;
  nr.fields = fields; nr.pre = pre; nr.post = post; nr.D = pre + 1 + post; nr.count = n;
  nr.sorted = sel;
  std::sort(nr.sorted.begin(), nr.sorted.end());
  nr.pos.resize(n);
  std::vector<mpcq_blackbox_rule> sorted_rules(n);
  for (int j = 0; j < n; ++j) {
    nr.pos[j] = (int)(std::lower_bound(nr.sorted.begin(), nr.sorted.end(), sel[j]) - nr.sorted.begin());
    sorted_rules[nr.pos[j]] = rules[j];
  }
  for (const Group& g : e->groups) {   // the part of the selection inside every group of mpcq_sim_steps, and inside the whole batch
    nr.glo.push_back((int)(std::lower_bound(nr.sorted.begin(), nr.sorted.end(), g.b0) - nr.sorted.begin()));
    nr.ghi.push_back((int)(std::lower_bound(nr.sorted.begin(), nr.sorted.end(), g.b0 + g.n) - nr.sorted.begin()));
  }
  // (a return from here on releases what `nr` holds by then; the engine's black box is touched by the last statements only)
  auto need = [&](auto& buf, size_t elems, const char* what) {
    return grow_or_fail(buf, elems, who + ": cannot allocate " + std::to_string(elems * sizeof(*buf.p)) + " bytes for " + what);
  };
  int rc = need(nr.d_sel, (size_t)n, "the selection");
  if (!rc) rc = need(nr.d_rules, (size_t)n, "the rules");
  if (!rc) rc = need(nr.d_int, 3 * (size_t)n, "the state");
  if (!rc) rc = need(nr.d_i64, 2 * (size_t)n, "the state");
  for (int f = 0; f < mpcq::record::NF && !rc; ++f) {
    if (!(fields >> f & 1)) continue;
    const size_t elems = (size_t)nr.D * n * mpcq::record::width(f, e->nb);
    rc = f == mpcq::record::F_SOLVER ? need(nr.d_solver, elems, "the solver field") : need(nr.d_f[f], elems, "a field's rings");
  }
  if (!rc && (fields & MPCQ_RECORD_DRAG)) rc = need(nr.d_snap, (size_t)n * mpcq::record::SNAP, "the drag snapshot");
  if (rc) return rc;
  if (hipMemcpyAsync(nr.d_sel.p, nr.sorted.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice, e->stream) != hipSuccess ||
      hipMemcpyAsync(nr.d_rules.p, sorted_rules.data(), (size_t)n * sizeof(mpcq_blackbox_rule), hipMemcpyHostToDevice, e->stream) != hipSuccess)
    return fail(MPCQ_ERR_DEVICE, who + ": copy of the selection and the rules failed");
  const bx::State st0 = nr.state();
  hipStream_t s = e->stream;
  hipLaunchKernelGGL(bx::init_kernel, dim3((n + 63) / 64), dim3(64), 0, s, st0, (const int*)nullptr, n, 0LL);
  if (hipGetLastError() != hipSuccess || hipStreamSynchronize(e->stream) != hipSuccess) return fail(MPCQ_ERR_DEVICE, who + ": the state could not be set");
  nr.on = true;
  e->bb = std::move(nr);
  return 0;
}
int mpcq_blackbox_info(mpcq_engine* e, int64_t* fired_period, int32_t* cause, int32_t* state, int32_t* rows, int32_t* fired_row, int64_t* periods) {
  ENTER(e);
  const BlackBox& r = e->bb;
  if (!r.on) return fail(MPCQ_ERR_STATE, "mpcq_blackbox_info: no black box running");
  if (periods) *periods = r.periods;
  if (!fired_period && !cause && !state && !rows && !fired_row) return 0;
  BoxState h;
  if (const int rc = box_state(e, h)) return rc;
  const size_t n = r.count;
  for (size_t j = 0; j < n; ++j) {   // caller's order
    const size_t k = r.pos[j];
    const BoxRows br = box_rows(r, h.ints[k], h.i64[k], h.i64[n + k]);
    if (fired_period) fired_period[j] = h.i64[k];
    if (cause) cause[j] = h.ints[n + k];
    if (state) state[j] = h.ints[k];
    if (rows) rows[j] = br.rows;
    if (fired_row) fired_row[j] = br.fired_row;
  }
  return 0;
}
int mpcq_blackbox_get(mpcq_engine* e, int32_t field, const int32_t* which, int32_t n, double* out) {
  ENTER(e);
  const BlackBox& r = e->bb;
  if (!r.on) return fail(MPCQ_ERR_STATE, "mpcq_blackbox_get: no black box running");
  if (field <= 0 || (field & (field - 1)) || !(field & r.fields) || field == MPCQ_RECORD_SOLVER)
    return fail(MPCQ_ERR_INVALID, "mpcq_blackbox_get: field is not one double field of this black box (MPCQ_RECORD_SOLVER: mpcq_blackbox_get_solver)");
  int f = 0;
  while (!(field >> f & 1)) ++f;
  return box_read(e, "mpcq_blackbox_get", (const double*)r.d_f[f].p, mpcq::record::width(f, e->nb), std::nan(""), which, n, out);
}
int mpcq_blackbox_get_solver(mpcq_engine* e, const int32_t* which, int32_t n, int32_t* out) {
  ENTER(e);
  const BlackBox& r = e->bb;
  if (!r.on) return fail(MPCQ_ERR_STATE, "mpcq_blackbox_get_solver: no black box running");
  if (!(r.fields & MPCQ_RECORD_SOLVER)) return fail(MPCQ_ERR_INVALID, "mpcq_blackbox_get_solver: MPCQ_RECORD_SOLVER is not a field of this black box");
  return box_read(e, "mpcq_blackbox_get_solver", (const int*)r.d_solver.p, 4, -1, which, n, (int*)out);
}
int mpcq_blackbox_get_periods(mpcq_engine* e, const int32_t* which, int32_t n, int64_t* out) {
  ENTER(e);
  const BlackBox& r = e->bb;
  if (!r.on) return fail(MPCQ_ERR_STATE, "mpcq_blackbox_get_periods: no black box running");
  std::vector<int> sel;
  if (const int rc = box_subset("mpcq_blackbox_get_periods", r, which, n, sel)) return rc;
  if (sel.empty()) return 0;
  if (!out) return fail(MPCQ_ERR_INVALID, "null argument");
  BoxState h;
  if (const int rc = box_state(e, h)) return rc;
  for (size_t i = 0; i < sel.size(); ++i) {
    const int j = sel[i];
    const BoxRows br = box_rows(r, h.ints[j], h.i64[j], h.i64[r.count + j]);
    for (int k = 0; k < r.D; ++k) out[i * r.D + k] = k < br.rows ? br.p0 + k : -1;
  }
  return 0;
}
int mpcq_blackbox_rearm(mpcq_engine* e, const int32_t* mask) {
  ENTER(e);
  BlackBox& r = e->bb;
  if (!r.on) return fail(MPCQ_ERR_STATE, "mpcq_blackbox_rearm: no black box running");
  const int* d_mask = nullptr;
  if (mask) {
    std::vector<int> m(r.count);
    for (int j = 0; j < r.count; ++j) m[r.pos[j]] = mask[j] != 0;
    if (const int rc = grow_or_fail(r.d_stage_int, (size_t)r.count, "mpcq_blackbox_rearm: cannot allocate the mask")) return rc;
    HIP_TRY(hipMemcpyAsync(r.d_stage_int.p, m.data(), m.size() * sizeof(int), hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));   // (m leaves scope)
    d_mask = r.d_stage_int.p;
  }
  return box_init(e, d_mask, r.periods);
}
int mpcq_blackbox_stop(mpcq_engine* e) { ENTER(e); return feature_stop(e, e->bb, "mpcq_blackbox_stop: no black box running"); }

// ---- flight scoreboard (mpcq_score.hpp; state, layout and launch: Score, score_launch)
namespace {
// table, cur, used and overflow to their start values on the engine's stream, and the period count to 0
int score_init(mpcq_engine* e) {
  Score& sc = e->sc;
  double* table = sc.d_table.p;
  int* ints = sc.d_int.p;
  const long B = e->B;
  const int F = sc.F;
  hipStream_t s = e->stream;
  hipLaunchKernelGGL(mpcq::score::score_init_kernel, dim3(mpcq::score::grid(B * F * mpcq::score::W)), dim3(mpcq::score::BLOCK), 0, s, table, ints, B, F);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(e->stream));
  sc.periods = 0;
  return 0;
}
}  // namespace
int mpcq_score_start(mpcq_engine* e, int32_t flights, int32_t tail_rows) {
  ENTER(e);
  if (flights < 1 || tail_rows < 0) return fail(MPCQ_ERR_INVALID, "mpcq_score_start: flights must be >= 1 and tail_rows >= 0");
  if ((size_t)e->B * (size_t)flights * mpcq::score::W > 0x7fffffffull) return fail(MPCQ_ERR_INVALID, "mpcq_score_start: table too large (B x flights x 16)");
  if (const int rc = needs_trajectories(e, "mpcq_score_start")) return rc;
  HIP_TRY(hipStreamSynchronize(e->stream));   // (launches of an mpcq_step_device_async may still write the table that is replaced)
  Score& sc = e->sc;
  sc.on = false;
  auto need = [](auto& buf, size_t elems) { return grow_or_fail(buf, elems, "mpcq_score_start: cannot allocate " + std::to_string(elems * sizeof(*buf.p)) + " bytes"); };
  int rc;
  if ((rc = need(sc.d_table, (size_t)e->B * flights * mpcq::score::W)) || (rc = need(sc.d_int, Score::n_ints(e->B)))) return rc;
  sc.F = flights; sc.tail_rows = tail_rows;
  if ((rc = score_init(e))) return rc;
  sc.on = true;
  return 0;
}
int mpcq_score_get(mpcq_engine* e, double* score, int32_t* flights, int32_t* overflow, int64_t* periods) {
  ENTER(e);
  const Score& sc = e->sc;
  if (!sc.on) return fail(MPCQ_ERR_STATE, "mpcq_score_get: no score running");
  const size_t B = e->B;
  if (score) HIP_TRY(hipMemcpyAsync(score, sc.d_table.p, B * sc.F * mpcq::score::W * sizeof(double), hipMemcpyDeviceToHost, e->stream));
  if (flights) HIP_TRY(hipMemcpyAsync(flights, sc.ints(B).used, B * sizeof(int), hipMemcpyDeviceToHost, e->stream));
  if (overflow) HIP_TRY(hipMemcpyAsync(overflow, sc.ints(B).overflow, B * sizeof(int), hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  if (periods) *periods = sc.periods;
  return 0;
}
int mpcq_score_clear(mpcq_engine* e) {
  ENTER(e);
  if (!e->sc.on) return fail(MPCQ_ERR_STATE, "mpcq_score_clear: no score running");
  return score_init(e);
}
int mpcq_score_stop(mpcq_engine* e) { ENTER(e); return feature_stop(e, e->sc, "mpcq_score_stop: no score running"); }

// ---- the fleet (mpcq_fleet.hpp; state and launch: Fleet, fleet_launch, in the place of the shared plant's launch: EngineT::plant_launch)
int mpcq_fleet_set(mpcq_engine* e, const mpcq_plant* plants, uint64_t plant_size, int64_t period0) {
  ENTER(e);
  namespace ft = mpcq::fleet;
  if (!plants) return fail(MPCQ_ERR_INVALID, "mpcq_fleet_set: plants is NULL");
  if (plant_size != sizeof(mpcq_plant))
    return fail(MPCQ_ERR_INVALID, "mpcq_fleet_set: plant_size " + std::to_string(plant_size) + " is not this library's sizeof(mpcq_plant) = " + std::to_string(sizeof(mpcq_plant)));
  if (period0 < -1) return fail(MPCQ_ERR_INVALID, "mpcq_fleet_set: period0 must be >= 0, or -1 to keep the fleet period");
  const size_t B = e->B;
  // every rule is checked before anything of the engine changes
  for (size_t b = 0; b < B; ++b) {
    const mpcq_plant& p = plants[b];
    auto bad = [&](const char* field, int i, const char* rule) {
      return fail(MPCQ_ERR_INVALID, "mpcq_fleet_set: quadrotor " + std::to_string(b) + ": " + field + (i >= 0 ? "[" + std::to_string(i) + "]" : std::string()) + " " + rule);
    };
    struct Field { const char* name; const double* v; int n; int rule; };   // rule 1: > 0; 2: in [0, 1]
    const Field fields[] = {{"mass", &p.mass, 1, 1}, {"J", p.J, 3, 1}, {"max_thrust", &p.max_thrust, 1, 1}, {"x_f", p.x_f, 4, 0}, {"y_f", p.y_f, 4, 0},
                            {"z_l_tau", p.z_l_tau, 4, 0}, {"rotor_drag", p.rotor_drag, 3, 0}, {"aero_drag", &p.aero_drag, 1, 0},
                            {"payload_mass", &p.payload_mass, 1, 0}, {"rotor_functionality", p.rotor_functionality, 4, 2}, {"f_d", p.f_d, 3, 0},
                            {"t_d", p.t_d, 3, 0}};
    for (const Field& f : fields)
      for (int i = 0; i < f.n; ++i) {
        const int at = f.n > 1 ? i : -1;
        if (!std::isfinite(f.v[i])) return bad(f.name, at, "is not finite");
        if (f.rule == 1 && !(f.v[i] > 0)) return bad(f.name, at, "must be > 0");
        if (f.rule == 2 && !(f.v[i] >= 0 && f.v[i] <= 1)) return bad(f.name, at, "must be in [0, 1]");
      }
  }
  std::vector<double> tab((size_t)ft::NF * B), row(ft::NF);
  for (size_t b = 0; b < B; ++b) {
    ft::pack(plants[b], e->cfg.g, row.data());
    for (int f = 0; f < ft::NF; ++f) tab[(size_t)f * B + b] = row[f];
  }
  Fleet& fl = e->fl;
  // The new table goes to a buffer of its own and takes the old one's place only once it is complete on the device: a failed allocation
  // or copy leaves the engine flying the table it had.
  DevBuf<double> fresh;
  if (const int rc = grow_or_fail(fresh, tab.size(), "mpcq_fleet_set: cannot allocate " + std::to_string(tab.size() * sizeof(double)) + " bytes")) return rc;
  HIP_TRY(hipMemcpyAsync(fresh.p, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));   // (behind it nothing the engine has enqueued reads the table that is replaced: the calls that launch the plant return synchronised)
  fl.d_tab = std::move(fresh);
  fl.plants.assign(plants, plants + B);
  if (period0 >= 0) fl.period = period0;
  else if (!fl.on) fl.period = 0;
  fl.on = true;
  return 0;
}
int mpcq_fleet_get(mpcq_engine* e, mpcq_plant* plants, uint64_t plant_size, int64_t* period) {
  ENTER(e);
  const Fleet& fl = e->fl;
  if (!fl.on) return fail(MPCQ_ERR_STATE, "mpcq_fleet_get: no fleet set");
  if (plant_size != sizeof(mpcq_plant)) return fail(MPCQ_ERR_INVALID, "mpcq_fleet_get: plant_size is not this library's sizeof(mpcq_plant)");
  if (plants) std::memcpy(plants, fl.plants.data(), fl.plants.size() * sizeof(mpcq_plant));
  if (period) *period = fl.period;
  return 0;
}
int mpcq_fleet_stop(mpcq_engine* e) { ENTER(e); return feature_stop(e, e->fl, "mpcq_fleet_stop: no fleet set"); }

// ---- the sensor (mpcq_sensor.hpp; state and launch: Sensor, sensor_launch, in front of every period of mpcq_sim_steps: EngineT::period)
int mpcq_sensor_start(mpcq_engine* e, const mpcq_sensor* sensors, uint64_t sensor_size, uint64_t seed, int64_t index0, int64_t period0, int32_t depth,
                      int32_t judge) {
  ENTER(e);
  namespace sr = mpcq::sensor;
  if (!sensors) return fail(MPCQ_ERR_INVALID, "mpcq_sensor_start: sensors is NULL");
  if (sensor_size != sizeof(mpcq_sensor))
    return fail(MPCQ_ERR_INVALID, "mpcq_sensor_start: sensor_size " + std::to_string(sensor_size) + " is not this library's sizeof(mpcq_sensor) = " + std::to_string(sizeof(mpcq_sensor)));
  if (depth < 1 || depth > sr::MAX_DEPTH) return fail(MPCQ_ERR_INVALID, "mpcq_sensor_start: depth " + std::to_string(depth) + " outside 1..32");
  if (judge != MPCQ_SENSOR_JUDGE_MEASURED && judge != MPCQ_SENSOR_JUDGE_TRUTH)
    return fail(MPCQ_ERR_INVALID, "mpcq_sensor_start: judge must be MPCQ_SENSOR_JUDGE_MEASURED (0) or MPCQ_SENSOR_JUDGE_TRUTH (1)");
  if (period0 < 0) return fail(MPCQ_ERR_INVALID, "mpcq_sensor_start: period0 must be >= 0");
  if (index0 < 0) return fail(MPCQ_ERR_INVALID, "mpcq_sensor_start: index0 must be >= 0");
  const size_t B = e->B;
  // every rule is checked before anything of the engine changes
  for (size_t b = 0; b < B; ++b) {
    const mpcq_sensor& s = sensors[b];
    auto bad = [&](const char* field, int i, const char* rule) {
      return fail(MPCQ_ERR_INVALID, "mpcq_sensor_start: quadrotor " + std::to_string(b) + ": " + field + (i >= 0 ? "[" + std::to_string(i) + "]" : std::string()) + " " + rule);
    };
    struct Field { const char* name; const double* v; int n; int rule; };   // rule 1: >= 0; 2: in [0, 1]
    const Field fields[] = {{"sigma_p", s.sigma_p, 3, 1}, {"sigma_att", s.sigma_att, 3, 1}, {"sigma_v", s.sigma_v, 3, 1}, {"sigma_r", s.sigma_r, 3, 1},
                            {"bias_p", s.bias_p, 3, 0}, {"bias_att", s.bias_att, 3, 0}, {"bias_v", s.bias_v, 3, 0}, {"bias_r", s.bias_r, 3, 0},
                            {"p_drop", &s.p_drop, 1, 2}};
    for (const Field& f : fields)
      for (int i = 0; i < f.n; ++i) {
        const int at = f.n > 1 ? i : -1;
        if (!std::isfinite(f.v[i])) return bad(f.name, at, "is not finite");
        if (f.rule == 1 && !(f.v[i] >= 0)) return bad(f.name, at, "must be >= 0");
        if (f.rule == 2 && !(f.v[i] >= 0 && f.v[i] <= 1)) return bad(f.name, at, "must be in [0, 1]");
      }
    if (s.delay < 0 || s.delay > depth - 1) return bad("delay", -1, ("must be in 0..depth-1 = 0.." + std::to_string(depth - 1)).c_str());
  }
  std::vector<double> tab((size_t)sr::NF * B), row(sr::NF);
  std::vector<long long> win((size_t)sr::NI * B);
  std::vector<int> ints(2 * B, 0);   // delay | age
  for (size_t b = 0; b < B; ++b) {
    sr::pack(sensors[b], row.data());
    for (int f = 0; f < sr::NF; ++f) tab[(size_t)f * B + b] = row[f];
    win[(size_t)sr::I_FROM * B + b] = sensors[b].out_from; win[(size_t)sr::I_TO * B + b] = sensors[b].out_to;
    ints[b] = sensors[b].delay;
  }
  // The new sensor is built beside the running one and takes its place only once it is complete on the device: a failed allocation or
  // copy leaves the engine measuring through the sensor it had.
  Sensor fresh;
  auto need = [](auto& buf, size_t elems) { return grow_or_fail(buf, elems, "mpcq_sensor_start: cannot allocate " + std::to_string(elems * sizeof(*buf.p)) + " bytes"); };
  int rc;
  if ((rc = need(fresh.d_tab, tab.size())) || (rc = need(fresh.d_win, win.size())) || (rc = need(fresh.d_int, ints.size())) ||
      (rc = need(fresh.d_ring, ((size_t)depth + 1) * 13 * B)))
    return rc;
  hipStream_t s = e->stream;
  HIP_TRY(hipMemcpyAsync(fresh.d_tab.p, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(fresh.d_win.p, win.data(), win.size() * sizeof(long long), hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(fresh.d_int.p, ints.data(), ints.size() * sizeof(int), hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemsetAsync(fresh.d_ring.p, 0, ((size_t)depth + 1) * 13 * B * sizeof(double), s));
  HIP_TRY(hipStreamSynchronize(s));   // (behind it nothing the engine has enqueued reads the buffers that are replaced)
  fresh.on = true;
  fresh.depth = depth; fresh.judge = judge; fresh.seed = seed;
  fresh.period = fresh.period0 = period0; fresh.index0 = index0;
  e->sn = std::move(fresh);
  return 0;
}
int mpcq_sensor_get(mpcq_engine* e, double* x_meas, int32_t* age, int64_t* period) {
  ENTER(e);
  const Sensor& sn = e->sn;
  if (!sn.on) return fail(MPCQ_ERR_STATE, "mpcq_sensor_get: no sensor running");
  const size_t B = e->B;
  if (x_meas) HIP_TRY(hipMemcpyAsync(x_meas, sn.out(B), 13 * B * sizeof(double), hipMemcpyDeviceToHost, e->stream));
  if (age) HIP_TRY(hipMemcpyAsync(age, sn.age(B), B * sizeof(int), hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  if (period) *period = sn.period;
  return 0;
}
int mpcq_sensor_sample(mpcq_engine* e, double* x_meas) {
  ENTER(e);
  if (!e->sn.on) return fail(MPCQ_ERR_STATE, "mpcq_sensor_sample: no sensor running");
  if (!x_meas) return fail(MPCQ_ERR_INVALID, "mpcq_sensor_sample: x_meas is NULL");
  sensor_launch(e->sn, e->view(), e->B, e->stream, 0, e->B, e->next_tick(false, false, true).nper);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(x_meas, e->sn.out(e->B), (size_t)13 * e->B * sizeof(double), hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  return 0;
}
int mpcq_sensor_stop(mpcq_engine* e) { ENTER(e); return feature_stop(e, e->sn, "mpcq_sensor_stop: no sensor running"); }

// ---- RGP read-out (mpcq_predict.hpp; predict_run).  The engine's stream is behind every group stream of mpcq_sim_steps when that call
// returns, and both calls run on it: they see the state after the last period.
namespace {
int predict_args(const char* who, const mpcq_engine* e, const double* xq, int32_t M, const double* mean, const double* var) {
  if (!xq) return fail(MPCQ_ERR_INVALID, std::string(who) + ": null query points");
  if (!mean && !var) return fail(MPCQ_ERR_INVALID, std::string(who) + ": mean and var are both NULL");
  if (M < 1 || M > mpcq::predict::MAX_M) return fail(MPCQ_ERR_INVALID, std::string(who) + ": M outside 1..4096");
  if (!e->nb) return fail(MPCQ_ERR_STATE, std::string(who) + ": engine has no RGP (nb = 0)");
  return 0;
}
}  // namespace
int mpcq_rgp_predict(mpcq_engine* e, const double* xq, int32_t M, int32_t per_quad, double* mean, double* var) {
  ENTER(e);
  if (per_quad != 0 && per_quad != 1) return fail(MPCQ_ERR_INVALID, "mpcq_rgp_predict: per_quad must be 0 or 1");
  if (const int rc = predict_args("mpcq_rgp_predict", e, xq, M, mean, var)) return rc;
  return e->rgp_predict(xq, M, per_quad, mean, var);
}
int mpcq_record_predict(mpcq_engine* e, const double* xq, int32_t M, int32_t row0, int32_t nrows, double* mean, double* var) {
  ENTER(e);
  const Recorder& r = e->rec;
  if (!r.on) return fail(MPCQ_ERR_STATE, "mpcq_record_predict: no active recording");
  if (const int rc = predict_args("mpcq_record_predict", e, xq, M, mean, var)) return rc;
  const bool fixed = (e->cfg.flags & MPCQ_FLAG_STATIC_GP) != 0;
  if (!(r.fields & MPCQ_RECORD_RGP_MU)) return fail(MPCQ_ERR_INVALID, "mpcq_record_predict: MPCQ_RECORD_RGP_MU was not recorded");
  if (var && !fixed && !(r.fields & MPCQ_RECORD_RGP_C)) return fail(MPCQ_ERR_INVALID, "mpcq_record_predict: var needs MPCQ_RECORD_RGP_C in the recording");
  if (row0 < 0 || nrows < 1 || (long long)row0 + nrows > r.rows) return fail(MPCQ_ERR_INVALID, "mpcq_record_predict: row window outside the rows recorded so far");
  const int nb = e->nb;
  return predict_run<double>(e, r.d_f[mpcq::record::F_MU].p, 3L * nb, fixed ? nullptr : r.d_f[mpcq::record::F_C].p, 3L * nb * nb, (size_t)r.count * nrows, r.pos.data(),
                             row0, nrows, r.count, xq, M, 0, mean, var);
}

// ---- device trainer (mpcq_train.hpp).  Both entry points run train_run on the engine's stream, as the RGP read-out does.
namespace {
// LDS a workgroup may ask for: the device's opt-in limit.  MPCQ_TRAIN_LDS_BYTES lowers it (tests and measurements: every residency arm
// at every basis size).
int train_lds_limit(int device, size_t* out) {
  size_t lim = 160 * 1024;
#ifndef MPCQ_EMU_BUILD
  int v = 0;
  if (hipDeviceGetAttribute(&v, hipDeviceAttributeSharedMemPerBlockOptin, device) != hipSuccess || v <= 0) {
    (void)hipGetLastError();
    HIP_TRY(hipDeviceGetAttribute(&v, hipDeviceAttributeMaxSharedMemoryPerBlock, device));
  }
  if (v > 0) lim = std::min(lim, (size_t)v);
#else
  (void)device;
#endif
  if (const char* s = getenv("MPCQ_TRAIN_LDS_BYTES")) {
    const long long v2 = atoll(s);
    if (v2 > 0 && (size_t)v2 < lim) lim = (size_t)v2;
  }
  *out = lim;
  return 0;
}
extern "C++" {   // (this part of the file has C linkage)
template <int MODE, bool RC, bool RK>
int train_launch(hipStream_t s, unsigned R, size_t lds, const mpcq::train::Args& a) {
  void (*k)(const mpcq::train::Args) = &mpcq::train::train_kernel<MODE, RC, RK>;
  HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(k, dim3(R), dim3(64), lds, s, a);
  HIP_TRY(hipGetLastError());
  return 0;
}
}
// the argument rules the two entry points share; *nb_out: the basis size trained with
int train_args(const char* who_, const mpcq_engine* e, const mpcq_train_spec* sp, const mpcq_train_out* out, int* nb_out) {
  const std::string who(who_);
  if (!sp || !out) return fail(MPCQ_ERR_INVALID, who + ": null spec or out");
  if (!out->mu && !out->C && !out->mu_eta && !out->C_eta && !out->Kx_inv) return fail(MPCQ_ERR_INVALID, who + ": every output is NULL");
  if (sp->mode != MPCQ_TRAIN_REGRESS && sp->mode != MPCQ_TRAIN_LEARN) return fail(MPCQ_ERR_INVALID, who + ": mode must be MPCQ_TRAIN_REGRESS or MPCQ_TRAIN_LEARN");
  if (sp->pair_next != 0 && sp->pair_next != 1) return fail(MPCQ_ERR_INVALID, who + ": pair_next must be 0 or 1");
  if (sp->nb < 0 || sp->nb > mpcq::train::MAX_NB) return fail(MPCQ_ERR_INVALID, who + ": nb outside 0..64");
  if (sp->nb > 0 && (!sp->basis || !sp->theta)) return fail(MPCQ_ERR_INVALID, who + ": nb > 0 needs basis and theta");
  if (sp->nb == 0 && (sp->basis || sp->theta)) return fail(MPCQ_ERR_INVALID, who + ": nb = 0 trains the engine's own model: basis and theta must be NULL");
  if (sp->mode == MPCQ_TRAIN_REGRESS && (out->mu_eta || out->C_eta || out->Kx_inv)) return fail(MPCQ_ERR_INVALID, who + ": mu_eta, C_eta and Kx_inv are outputs of MPCQ_TRAIN_LEARN");
  if (sp->nb > 0)
    for (int d = 0; d < 3; ++d)
      if (!(sp->theta[d * 3] > 0)) return fail(MPCQ_ERR_INVALID, who + ": theta: length scale must be > 0");
  if (sp->nb == 0 && !e->nb) return fail(MPCQ_ERR_STATE, who + ": engine has no RGP (nb = 0)");
  if (sp->nb == 0 && e->nb > mpcq::train::MAX_NB) return fail(MPCQ_ERR_INVALID, who + ": the engine's basis is larger than 64");
  *nb_out = sp->nb ? sp->nb : e->nb;
  return 0;
}
// v, a: device pointers to sample 0 (inputs, targets); sample k of stream s, axis d at [(pos ? pos[s] : s) * stream_stride + k * step_stride + d].
// T counts the samples as stored; with pair_next the targets move one step on and T - 1 samples are walked.
int train_run(mpcq_engine* e, const mpcq_train_spec* sp, int nb, const double* v, const double* a, long stream_stride, long step_stride,
              const int* pos_host, int S, int T, const mpcq_train_out* out) {
  namespace tn = mpcq::train;
  mpcq_engine::TrainScratch& tr = e->tr;
  hipStream_t s = e->stream;
  const bool learn = sp->mode == MPCQ_TRAIN_LEARN, own = sp->nb == 0;
  const size_t n = nb, nn = n * n, R = (size_t)S * 3;
  if (R > 0x7fffffffull) return fail(MPCQ_ERR_INVALID, "RGP training: too many streams for one call");
  auto need = [](auto& buf, size_t elems) { return grow_or_fail(buf, elems, "RGP training: cannot allocate " + std::to_string(elems * sizeof(*buf.p)) + " bytes"); };
  int rc;
  // the model on the device: theta | K_x (the start value of C) | basis | K_x^-1
  const double* basis_h = own ? e->basis.data() : sp->basis;
  const double* theta_h = own ? e->theta.data() : sp->theta;
  std::vector<double> hm(9 + 3 * nn + (own ? 0 : 3 * n + 3 * nn), 0.0);
  std::copy(theta_h, theta_h + 9, hm.begin());
  if (!learn)   // (LEARN builds its start values on the device, as mpcq_learn_create does)
    for (int d = 0; d < 3; ++d) {
      std::vector<double> K, Ki;
      if (!rgp_axis_constants(basis_h + d * n, nb, theta_h[3 * d], theta_h[3 * d + 1], theta_h[3 * d + 2], K, Ki))
        return fail(MPCQ_ERR_INVALID, "RGP training: K_x is not positive definite");
      std::copy(K.begin(), K.end(), hm.begin() + 9 + d * nn);
      if (!own) std::copy(Ki.begin(), Ki.end(), hm.begin() + 9 + 3 * nn + 3 * n + d * nn);
    }
  if (!own) std::copy(basis_h, basis_h + 3 * n, hm.begin() + 9 + 3 * nn);
  if ((rc = need(tr.model, hm.size()))) return rc;
  if (own && (rc = rgp_model_on_device(e))) return rc;
  HIP_TRY(hipMemcpyAsync(tr.model.p, hm.data(), hm.size() * sizeof(double), hipMemcpyHostToDevice, s));
  if (pos_host) {
    if ((rc = need(tr.pos, (size_t)S))) return rc;
    HIP_TRY(hipMemcpyAsync(tr.pos.p, pos_host, (size_t)S * sizeof(int), hipMemcpyHostToDevice, s));
  }
  const size_t o_mu = 0, o_C = o_mu + R * n, o_eta = o_C + R * nn, o_Ce = o_eta + R * 3, o_K = o_Ce + R * 9;
  if ((rc = need(tr.out, learn ? o_K + R * nn : o_eta))) return rc;
  tn::Args g;
  std::memset(&g, 0, sizeof(g));
  g.nb = nb; g.T = sp->pair_next ? T - 1 : T;
  g.v = v; g.a = sp->pair_next ? a + step_stride : a;
  g.stream_stride = stream_stride; g.step_stride = step_stride;
  g.pos = pos_host ? tr.pos.p : nullptr;
  g.theta = tr.model.p;
  g.C0 = tr.model.p + 9;
  g.basis = own ? e->pr.basis.p : tr.model.p + 9 + 3 * nn;
  g.K0 = own ? e->pr.Kinv.p : tr.model.p + 9 + 3 * nn + 3 * n;
  g.mu = tr.out.p + o_mu; g.C = tr.out.p + o_C;
  if (learn) { g.mu_eta = tr.out.p + o_eta; g.C_eta = tr.out.p + o_Ce; g.Kinv = tr.out.p + o_K; }
  // residency: the largest of {C and K_x^-1, C, neither} in LDS that the limit allows
  size_t limit = 0;
  if ((rc = train_lds_limit(e->cfg.device, &limit))) return rc;
  int arm = -1;
  size_t lds = 0;
  for (int k = 0; k < 3 && arm < 0; ++k) {
    lds = (size_t)tn::layout(nb, sp->mode, k < 2, k < 1).total * sizeof(double);
    if (lds <= limit) arm = k;
  }
  if (arm < 0) return fail(MPCQ_ERR_DEVICE, "RGP training: " + std::to_string(lds) + " bytes of LDS per workgroup needed, " + std::to_string(limit) + " available");
  const unsigned Ru = (unsigned)R;
  if (learn) rc = arm == 0 ? train_launch<tn::LEARN, true, true>(s, Ru, lds, g) : arm == 1 ? train_launch<tn::LEARN, true, false>(s, Ru, lds, g) : train_launch<tn::LEARN, false, false>(s, Ru, lds, g);
  else rc = arm == 0 ? train_launch<tn::REGRESS, true, true>(s, Ru, lds, g) : arm == 1 ? train_launch<tn::REGRESS, true, false>(s, Ru, lds, g) : train_launch<tn::REGRESS, false, false>(s, Ru, lds, g);
  if (rc) return rc;
  if (out->mu) HIP_TRY(hipMemcpyAsync(out->mu, g.mu, R * n * sizeof(double), hipMemcpyDeviceToHost, s));
  if (out->C) HIP_TRY(hipMemcpyAsync(out->C, g.C, R * nn * sizeof(double), hipMemcpyDeviceToHost, s));
  if (out->mu_eta) HIP_TRY(hipMemcpyAsync(out->mu_eta, g.mu_eta, R * 3 * sizeof(double), hipMemcpyDeviceToHost, s));
  if (out->C_eta) HIP_TRY(hipMemcpyAsync(out->C_eta, g.C_eta, R * 9 * sizeof(double), hipMemcpyDeviceToHost, s));
  if (out->Kx_inv) HIP_TRY(hipMemcpyAsync(out->Kx_inv, g.Kinv, R * nn * sizeof(double), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return 0;
}
}  // namespace
int mpcq_rgp_train(mpcq_engine* e, const mpcq_train_spec* sp, const double* v_body, const double* a_drag, int32_t S, int32_t T, mpcq_train_out* out) {
  ENTER(e);
  int nb = 0;
  if (const int rc = train_args("mpcq_rgp_train", e, sp, out, &nb)) return rc;
  if (!v_body || !a_drag) return fail(MPCQ_ERR_INVALID, "mpcq_rgp_train: null samples");
  if (S < 1) return fail(MPCQ_ERR_INVALID, "mpcq_rgp_train: S must be >= 1");
  if (T < 1 + sp->pair_next) return fail(MPCQ_ERR_INVALID, "mpcq_rgp_train: T must be >= 1 (>= 2 with pair_next)");
  const size_t cnt = (size_t)S * T * 3;
  if (const int rc = grow_or_fail(e->tr.in, 2 * cnt, "mpcq_rgp_train: cannot allocate the sample buffer")) return rc;
  HIP_TRY(hipMemcpyAsync(e->tr.in.p, v_body, cnt * sizeof(double), hipMemcpyHostToDevice, e->stream));
  HIP_TRY(hipMemcpyAsync(e->tr.in.p + cnt, a_drag, cnt * sizeof(double), hipMemcpyHostToDevice, e->stream));
  return train_run(e, sp, nb, e->tr.in.p, e->tr.in.p + cnt, 3L * T, 3, nullptr, S, T, out);
}
int mpcq_record_train(mpcq_engine* e, const mpcq_train_spec* sp, int32_t row0, int32_t nrows, mpcq_train_out* out) {
  ENTER(e);
  const Recorder& r = e->rec;
  if (!r.on) return fail(MPCQ_ERR_STATE, "mpcq_record_train: no active recording");
  int nb = 0;
  if (const int rc = train_args("mpcq_record_train", e, sp, out, &nb)) return rc;
  if (!(r.fields & MPCQ_RECORD_DRAG)) return fail(MPCQ_ERR_INVALID, "mpcq_record_train: MPCQ_RECORD_DRAG was not recorded");
  if (row0 < 0 || nrows < 1 + sp->pair_next || (long long)row0 + nrows > r.rows)
    return fail(MPCQ_ERR_INVALID, "mpcq_record_train: row window outside the rows recorded so far (nrows >= 1, >= 2 with pair_next)");
  const double* slab = r.d_f[mpcq::record::F_DRAG].p + (size_t)row0 * r.count * 6;
  return train_run(e, sp, nb, slab, slab + 3, 6, 6L * r.count, r.pos.data(), r.count, nrows, out);
}

int mpcq_get_trajectories(mpcq_engine* e, double* traj, int32_t* len) {
  ENTER(e);
  if (const int rc = needs_trajectories(e, "mpcq_get_trajectories")) return rc;
  const EngineView t = e->view();
  if (traj) HIP_TRY(hipMemcpyAsync(traj, t.traj, (size_t)e->B * t.Tmax * 13 * sizeof(double), hipMemcpyDeviceToHost, e->stream));
  if (len) HIP_TRY(hipMemcpyAsync(len, t.len, (size_t)e->B * sizeof(int), hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  return 0;
}

}  // extern "C"

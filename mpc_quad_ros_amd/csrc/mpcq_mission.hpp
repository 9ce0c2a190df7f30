// mpcq_mission.hpp — device missions (mpcq_mission_set): a queue of upcoming flights per quadrotor and one launch behind every period that
// installs the next flight for whoever just finished, with no host in between.  Included from mpcq_api.hip after mpcq_replan_nl.hpp and
// mpcq_circle.hpp.
//
// The flight itself is mpcq_replan's (plan_linear), mpcq_replan_nonlinear's (plan_nonlinear) or mpcq_replan_circle's (plan_circle), as the
// leg's entry of the legs table says and with that entry's limits: the same device function the host calls run, so a mission plans bit
// for bit what the host loop plans that runs, behind every `sim_steps(1)`, over the quadrotors due (finished & (leg < L)):
// `replan_circle(radius, v_max, mask = circle legs due)`, then `replan(wp[b, leg[b]], v, a, mask = waypoint legs due with these limits)`
// once per distinct pair of limits (v, a) among them, then `leg += 1`.  (mpcq_mission_set: no circle leg and one pair of limits, so one replan.)
//  * The grid does not depend on how many quadrotors finished: workgroups of one wavefront, about one per 16 quadrotors of the range.
//  * Every workgroup sweeps the flags of the whole range once, 64 per load, from a start point of its own (its share comes first), and plans
//    the candidates it wins one after another.  A candidate is won by a compare-and-swap on its ticket claim[b] (old value -> this period's
//    token), so quadrotors that finish in the same period spread over the workgroups that have nothing else to do -- neighbours do not
//    serialise on the workgroup whose share they are in -- and nobody is planned twice: a sweep that still sees the flag of a quadrotor
//    another workgroup has installed meanwhile loses the ticket.
//  * Per consumed leg lane 0 writes the leg counter, installed, last_code, leg_code, leg_period and (nonlinear, flight installed) info.
// Everything is wave-uniform per quadrotor, as in replan_kernel.
#pragma once

namespace mpcq {
namespace replan {

struct MissionArgs {
  double* traj; int Tmax; int *lens, *idx, *finished;   // the trajectory slots (EngineView)
  const double* start;        // [B,13]: the plant state behind the period's update, or the period's measurement
  const double* wp;           // [B,L,n_wp,3] (not read for a circle leg; nullptr if the queue has no waypoint leg)
  const mpcq_leg* legs;       // [B,L]: kind, limits and radius of every leg (mpcq_mission_set: the same waypoint leg everywhere)
  int L, n_wp, order;
  double dt;
  int b0, n;                  // the range [b0, b0 + n) of this launch (a group of mpcq_sim_steps, or the batch)
  int period;                 // period number since mpcq_mission_set
  int *leg, *installed, *last_code, *claim;   // [B]
  int *leg_code, *leg_period;                 // [B,L]
  double* info;               // [B,6] (nonlinear)
};

template <typename LdsT> struct MissionLds {
  LdsT plan;
  double info[6];
  int won, leg;
};

constexpr int MISSION_SHARE = 16, MISSION_MAX_GRID = 512;
inline int mission_grid(int n) {
  const int g = (n + MISSION_SHARE - 1) / MISSION_SHARE;
  return g < 1 ? 1 : (g > MISSION_MAX_GRID ? MISSION_MAX_GRID : g);
}

// a waypoint leg with the limits of its table entry
__device__ inline int mission_plan(MissionLds<Lds>& M, const MissionArgs& a, const mpcq_nl::Opts&, int b, const double* wp_b, double v_max, double a_max) {
  return plan_linear(M.plan, a.traj, a.Tmax, a.lens, a.idx, a.finished, b, a.start + (size_t)b * NX, wp_b, a.n_wp, v_max, a_max, a.order, a.dt);
}
__device__ inline int mission_plan(MissionLds<NlLds>& M, const MissionArgs& a, const mpcq_nl::Opts& o, int b, const double* wp_b, double v_max, double a_max) {
  return plan_nonlinear(M.plan, a.traj, a.Tmax, a.lens, a.idx, a.finished, b, a.start + (size_t)b * NX, wp_b, a.n_wp, v_max, a_max, a.order, a.dt, o,
                        M.info, nullptr, nullptr);
}
// the LDS a circle leg works in: the linear generator's
__device__ inline Lds& mission_circle_lds(Lds& S) { return S; }
__device__ inline Lds& mission_circle_lds(NlLds& L) { return L.base; }

template <typename LdsT>
__global__ __launch_bounds__(64) void mission_kernel(const MissionArgs a, const mpcq_nl::Opts o) {
  MissionLds<LdsT>& M = *reinterpret_cast<MissionLds<LdsT>*>(smem_raw);
  const int lane = threadIdx.x, w = blockIdx.x, G = gridDim.x;
  const int chunks = (a.n + 63) / 64, span = chunks * 64, token = a.period + 1;
  const int p0 = (int)(((long long)w * a.n) / G);   // where this workgroup's sweep starts: its own share
  for (int c = 0; c < chunks; ++c) {
    int j = p0 + c * 64 + lane;   // place in the range, cyclic over `span`
    if (j >= span) j -= span;
    const int b = a.b0 + j;
    const bool cand = j < a.n && a.finished[b] != 0 && a.leg[b] < a.L;
    int last = -1;
    for (;;) {   // the candidates of these 64, in lane order
      const int next = (int)wave_min((cand && lane > last) ? (double)lane : 1e9);
      if (next >= 64) break;
      last = next;
      int jn = p0 + c * 64 + next;
      if (jn >= span) jn -= span;
      const int bn = a.b0 + jn;
      __syncthreads();
      if (lane == 0) {
        const int seen = a.claim[bn];
        M.won = seen != token && atomicCAS(a.claim + bn, seen, token) == seen;
        M.leg = a.leg[bn];
      }
      __syncthreads();
      const int leg = M.leg;
      if (!M.won || leg >= a.L) continue;
      const mpcq_leg lg = a.legs[(size_t)bn * a.L + leg];   // (every lane loads the same entry)
      const bool circle = lg.kind == MPCQ_LEG_CIRCLE;
      const int code = circle ? plan_circle(mission_circle_lds(M.plan), a.traj, a.Tmax, a.lens, a.idx, a.finished, bn, a.start + (size_t)bn * NX, lg.radius,
                                            lg.v_max, CIRCLE_ACC_DEC, a.dt, 0.0)
                              : mission_plan(M, a, o, bn, a.wp + ((size_t)bn * a.L + leg) * a.n_wp * 3, lg.v_max, lg.a_max);
      __syncthreads();
      // the leg is consumed whatever the code (a negative one left trajectory, cursor and flag as they were: the next period tries the next leg)
      if (lane == 0) {
        a.leg[bn] = leg + 1;
        a.last_code[bn] = code;
        a.leg_code[(size_t)bn * a.L + leg] = code;
        a.leg_period[(size_t)bn * a.L + leg] = a.period;
        if (code == DONE) a.installed[bn] = a.installed[bn] + 1;
      }
      if (a.info && code == DONE && lane < 6) a.info[(size_t)bn * 6 + lane] = circle ? __builtin_nan("") : M.info[lane];   // (a circle has no info row)
    }
  }
}

}  // namespace replan
}  // namespace mpcq

"""Rate of the device flight generator (mpcq_replan) and of continuous operation built on it.

1. `replan`: mpcq_replan with every quadrotor selected, 3 waypoints, v = a = 12, B = 1024 and 8192: median host-clock wall time of
   20 blocking calls after warm-up, next to the host generator (libmpcq_traj.so: mpcq_minsnap_generate_order + mpcq_minsnap_sample)
   on one CPU thread for the same flights.  (Kernel time: run this under `rocprofv3 --kernel-trace --stats` with --only-replan.)
2. `continuous`: the bench workload shape (configs[1] N = 20, RGP 10, fp64) at B = 1024 and 8192.  Continuous operation = every
   quadrotor starts on a two-row hover reference at the bench's start state and from then on flies `sim_steps(R)` + `replan(mask=None)`
   through the waypoints of trajectories.flight_waypoints (the draws of the pre-chained missions), 600-period pre-roll; next to it
   plain `sim_steps` on the pre-chained missions of bench.workload, the two timed in alternating blocks in one process.

usage: python tools/replan_rate.py [--out profiles/replan_rate.json] [--only-replan] [--batches 1024,8192]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from mpc_quad_ros_amd.engine import REPLAN_DONE, REPLAN_TOO_LONG, Engine  # noqa: E402
from mpc_quad_ros_amd.params import EngineConfig, hummingbird, rgp_basis_linspace  # noqa: E402
from mpc_quad_ros_amd.trajectories import flight_waypoints, minsnap_pieces_order, sample_polynomial_trajectory_native  # noqa: E402

SEED, V, A, N, NB, LEGS = 7, 12.0, 12.0, 20, 10, 12


def config(B):
    return EngineConfig(batch=B, N=N, T=1.0, quad=hummingbird(), nb=NB, basis=rgp_basis_linspace(12.0, NB), theta=[1.0, 0.1, 0.1], dt_pred=0.01)


def waypoint_bank(B, legs):
    return np.stack([np.stack([flight_waypoints(SEED, i, leg) for i in range(B)]) for leg in range(legs)])   # [legs, B, 3, 3]


def replan_rate(B, Tmax=1600, calls=20, warm=3):
    rng = np.random.default_rng(B)
    start = rng.uniform(-5, 5, (B, 3)) + [0, 0, 7.5]
    wp = waypoint_bank(B, 1)[0]
    e = Engine(config(B))
    traj = np.zeros((B, Tmax, 13)); traj[:, :, 3] = 1
    e.set_trajectories(traj, np.full(B, 1, np.int32))
    mask = np.ones(B, np.int32)
    for _ in range(warm):
        codes = e.replan(wp, V, A, start=start, mask=mask)
    times = []
    for _ in range(calls):
        t0 = time.perf_counter()
        e.replan(wp, V, A, start=start, mask=mask)
        times.append(time.perf_counter() - t0)
    _, lens = e.get_trajectories()
    e.close()
    t0 = time.perf_counter()
    rows = 0
    for b in range(B):
        x = sample_polynomial_trajectory_native(minsnap_pieces_order(np.vstack([start[b], wp[b]]), V, A, 4))[0]
        rows += len(x)
    host = time.perf_counter() - t0
    med = float(np.median(times))
    return {"batch": B, "waypoints": 3, "v_max": V, "a_max": A, "Tmax": Tmax, "calls": calls, "device_wall_median_s": med,
            "device_wall_min_s": float(np.min(times)), "device_wall_max_s": float(np.max(times)),
            "done": int((codes == REPLAN_DONE).sum()), "too_long": int((codes == REPLAN_TOO_LONG).sum()), "mean_rows": float(lens.mean()),
            "host_one_thread_s": host, "host_per_flight_ms": 1e3 * host / B, "host_rows_mean": rows / B, "speedup_vs_host_thread": host / med}


PREROLL, BLOCK, ROUNDS = 600, 100, 3


def continuous_rate(B, refs, preroll=PREROLL, block=BLOCK, rounds=ROUNDS, Tmax=1600):
    n_sub = 2
    bank = waypoint_bank(B, LEGS)
    ep, _ = bench.make_engine(B, N, NB, 0, 0, 0, SEED, refs=refs)
    ec = Engine(config(B))
    x0 = np.tile(bench.X0, (B, 1))
    hover = np.repeat(x0[:, None, :], Tmax, axis=1)
    hover[:, :, 7:] = 0
    ec.set_trajectories(hover, np.full(B, 2, np.int32))     # (a flight finishes when idx + 1 == len after the step: two rows)
    ec.sim_reset(x0)
    leg = np.zeros(B, np.int64)
    stats = {"flights": 0, "too_long": 0, "other": 0}
    ar = np.arange(B)

    def cont(K, R):
        for _ in range(K // R):
            ec.sim_steps(R, n_sub, 5e-3)
            codes = ec.replan(bank[np.minimum(leg, LEGS - 1), ar], V, A)
            done = codes == REPLAN_DONE
            leg[done] += 1
            stats["flights"] += int(done.sum()); stats["too_long"] += int((codes == REPLAN_TOO_LONG).sum())
            stats["other"] += int(((codes != REPLAN_DONE) & (codes != 1) & (codes != REPLAN_TOO_LONG)).sum())

    ep.sim_run(preroll, n_sub, 5e-3)
    cont(preroll, 10)
    pre_flights = stats["flights"]
    rates = {"R1": [], "R10": [], "prechained": []}
    for _ in range(rounds):
        for key in ("R1", "R10", "prechained"):
            t0 = time.perf_counter()
            if key == "prechained":
                ep.sim_steps(block, n_sub, 5e-3)
            else:
                cont(block, 1 if key == "R1" else 10)
            rates[key].append(B * block / (time.perf_counter() - t0))
    _, lens = ec.get_trajectories()
    ep.close(); ec.close()
    med = {k: float(np.median(v)) for k, v in rates.items()}
    return {"batch": B, "N": N, "nb": NB, "precision": "fp64", "n_sub": n_sub, "preroll": preroll, "block_periods": block, "rounds": rounds,
            "steps_per_s_median": med, "steps_per_s_all": rates,
            "ratio_R10_to_prechained": med["R10"] / med["prechained"], "ratio_R1_to_prechained": med["R1"] / med["prechained"],
            "flights_replanned_preroll": pre_flights, "flights_replanned_total": stats["flights"], "too_long": stats["too_long"],
            "other_negative": stats["other"], "max_legs_used": int(leg.max()), "mean_len_at_end": float(lens.mean())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--only-replan", action="store_true")
    ap.add_argument("--batches", default="1024,8192")
    args = ap.parse_args()
    batches = [int(b) for b in args.batches.split(",")]
    from mpc_quad_ros_amd import _lib
    out = {"tool": "tools/replan_rate.py", "library": _lib.load().mpcq_version().decode(), "source_sha16": bench.kernel_source_sha16(),
           "replan": [], "continuous": []}
    if not args.only_replan:
        # pre-chained missions of every batch first: bench.workload forks worker processes, before this process touches the GPU
        refs = {B: bench.workload(SEED, 0, B, PREROLL + ROUNDS * BLOCK + 10) for B in batches}
        for B in batches:
            out["continuous"].append(continuous_rate(B, refs.pop(B)))
            print(json.dumps(out["continuous"][-1]), flush=True)
    for B in batches:
        out["replan"].append(replan_rate(B))
        print(json.dumps(out["replan"][-1]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()

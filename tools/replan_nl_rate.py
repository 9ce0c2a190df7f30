"""Rate of the device nonlinear flight generator (mpcq_replan_nonlinear) against the host library on one thread.

mpcq_replan_nonlinear with every quadrotor selected, 3 waypoints (trajectories.flight_waypoints), v = a = 12, jerk cost, default options,
B = 1024 and 8192: median host-clock wall time of blocking calls after warm-up, the evaluations used per flight (info column 2: median,
max).  Next to it the host generator (libmpcq_traj.so mpcq_minsnap_nonlinear + mpcq_minsnap_sample) on one CPU thread, timed on the first
256 flights and reported per flight.  Kernel time: run again under `rocprofv3 --kernel-trace --stats -- python tools/replan_nl_rate.py
--calls 3` (a run of its own; the stats CSV goes to profiles/).

usage: python tools/replan_nl_rate.py [--out profiles/replan_nl_rate.json] [--batches 1024,8192] [--calls 10] [--host-flights 256]
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
from mpc_quad_ros_amd.params import EngineConfig, hummingbird  # noqa: E402
from mpc_quad_ros_amd.trajectories import flight_waypoints, minsnap_pieces_nonlinear, sample_polynomial_trajectory_native  # noqa: E402

SEED, V, A, ORDER = 7, 12.0, 12.0, 3


def rate(B, calls, host_flights, Tmax=2400, warm=2):
    rng = np.random.default_rng(B)
    start = rng.uniform(-5, 5, (B, 3)) + [0, 0, 7.5]
    wp = np.stack([flight_waypoints(SEED, i, 0) for i in range(B)])
    e = Engine(EngineConfig(batch=B, N=10, T=1.0, quad=hummingbird(), dt_pred=0.01))
    traj = np.zeros((B, Tmax, 13)); traj[:, :, 3] = 1
    e.set_trajectories(traj, np.full(B, 1, np.int32))
    mask = np.ones(B, np.int32)
    for _ in range(warm):
        codes, info = e.replan_nonlinear(wp, V, A, 0.01, ORDER, start=start, mask=mask)
    times = []
    for _ in range(calls):
        t0 = time.perf_counter()
        e.replan_nonlinear(wp, V, A, 0.01, ORDER, start=start, mask=mask)
        times.append(time.perf_counter() - t0)
    e.close()
    h = min(host_flights, B)
    t0 = time.perf_counter()
    for b in range(h):
        pieces, _, _ = minsnap_pieces_nonlinear(np.vstack([start[b], wp[b]]), V, A, ORDER)
        sample_polynomial_trajectory_native(pieces, 0.01)
    host_per_flight = (time.perf_counter() - t0) / h
    med = float(np.median(times))
    ok = np.isfinite(info[:, 2])
    return {"batch": B, "waypoints": 3, "v_max": V, "a_max": A, "derivative_to_optimize": ORDER, "options": "defaults", "calls": calls,
            "device_wall_median_s": med, "device_wall_min_s": float(np.min(times)), "device_wall_max_s": float(np.max(times)),
            "done": int((codes == REPLAN_DONE).sum()), "too_long": int((codes == REPLAN_TOO_LONG).sum()),
            "evaluations_median": float(np.median(info[ok, 2])), "evaluations_max": float(info[ok, 2].max()),
            "duration_mean_s": float(info[ok, 3].mean()), "host_flights_timed": h, "host_per_flight_ms": 1e3 * host_per_flight,
            "host_one_thread_all_flights_s_extrapolated": host_per_flight * B, "speedup_vs_host_thread": host_per_flight * B / med}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batches", default="1024,8192")
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--host-flights", type=int, default=256)
    args = ap.parse_args()
    from mpc_quad_ros_amd import _lib
    out = {"tool": "tools/replan_nl_rate.py", "library": _lib.load().mpcq_version().decode(), "source_sha16": bench.kernel_source_sha16(),
           "replan_nonlinear": []}
    for B in (int(b) for b in args.batches.split(",")):
        out["replan_nonlinear"].append(rate(B, args.calls, args.host_flights))
        print(json.dumps(out["replan_nonlinear"][-1]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()

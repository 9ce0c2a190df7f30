"""Cost of the flight scoreboard (mpcq_score_*) on the bench workload (configs[1] shape: N = 20, RGP 10, fp64, pre-chained missions).

For B = 1024 (one group) and 8192 (two groups, split plant: the engine's automatic choices) one engine flies blocks of
`sim_steps(STEPS)`; the blocks alternate (in rotating order) between no score, `score_start(flights=8)` and -- for the kernel times, next
to it -- the flight recorder with its default fields for every quadrotor (started before the block and stopped behind it, outside the
timed region).  Neither changes anything in the flight, so the three modes fly the same kind of periods.  Rate = B x STEPS / host-clock
wall time of the blocking call; median over ROUNDS blocks per mode after WARM warm-up periods.  (Device time of score_kernel and
record_kernel: run this under `rocprofv3 --kernel-trace --stats` with --rounds 1.)

usage: python tools/score_rate.py [--out profiles/score_rate.json] [--batches 1024,8192] [--rounds 6]
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

SEED, N, NB, STEPS, WARM, N_SUB, FLIGHTS = 7, 20, 10, 200, 40, 2, 8
MODES = ("off", "score", "record")


def rate(B, refs, rounds):
    e, _ = bench.make_engine(B, N, NB, 0, 0, 0, SEED, refs=refs)
    e.sim_steps(WARM, N_SUB, 5e-3)
    rates = {k: [] for k in MODES}
    keys = list(MODES)
    for r in range(rounds):
        for key in keys[r % 3:] + keys[:r % 3]:   # (the order rotates: every mode flies every position of a round equally often)
            if key == "score":
                e.score_start(FLIGHTS)
            if key == "record":
                e.record_start(capacity=STEPS)
            t0 = time.perf_counter()
            e.sim_steps(STEPS, N_SUB, 5e-3)
            rates[key].append(B * STEPS / (time.perf_counter() - t0))
            if key == "score":
                sc = e.score_get()
                assert sc["periods"] == STEPS and ((sc["steps"] + sc["tail_steps"]).sum(axis=1) + sc["overflow"] == STEPS).all()
                e.score_stop()
            if key == "record":
                assert e.record_info()[0] == STEPS
                e.record_stop()
    groups = e.get_groups()
    e.close()
    med = {k: float(np.median(v)) for k, v in rates.items()}
    return {"batch": B, "N": N, "nb": NB, "groups": groups, "steps_per_call": STEPS, "rounds": rounds, "flights": FLIGHTS,
            "steps_per_s_median": med, "steps_per_s_all": rates, "cost_vs_off": {k: 1 - med[k] / med["off"] for k in ("score", "record")},
            # per quadrotor and period: the slot row read and written, the cursor / length / flags and 12 entries of measurement and reference
            "score_bytes_per_period": B * (2 * 128 + 7 * 4 + 13 * 8), "table_bytes": B * FLIGHTS * 128}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batches", default="1024,8192")
    ap.add_argument("--rounds", type=int, default=6)
    args = ap.parse_args()
    batches = [int(b) for b in args.batches.split(",")]
    from mpc_quad_ros_amd import _lib
    out = {"tool": "tools/score_rate.py", "library": _lib.load().mpcq_version().decode(), "source_sha16": bench.kernel_source_sha16(),
           "rates": []}
    # pre-chained missions first: bench.workload forks worker processes, before this process touches the GPU
    refs = {B: bench.workload(SEED, 0, B, WARM + 3 * args.rounds * STEPS + 10) for B in batches}
    for B in batches:
        out["rates"].append(rate(B, refs.pop(B), args.rounds))
        print(json.dumps(out["rates"][-1]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()

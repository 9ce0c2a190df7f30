"""Cost of the flight recorder (mpcq_record_*) on the bench workload (configs[1] shape: N = 20, RGP 10, fp64, pre-chained missions).

For B = 1024 (one group) and 8192 (two groups, split plant: the engine's automatic choices) one engine flies blocks of
`sim_steps(STEPS)`; the blocks alternate (in rotating order) between recording off, the default fields of Engine.record_start for every quadrotor with
every = 1, and the same plus rgp_C (record_start before the block, record_stop behind it, outside the timed region).  Recording
changes nothing in the flight, so the three modes fly the same kind of periods.  Rate = B x STEPS / host-clock wall time of the
blocking call; median over ROUNDS blocks per mode after WARM warm-up periods.  (Kernel time of the record launches: run this
under `rocprofv3 --kernel-trace --stats` with --rounds 1.)

usage: python tools/record_rate.py [--out profiles/record_rate.json] [--batches 1024,8192] [--rounds 6]
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
from mpc_quad_ros_amd.engine import RECORD_DEFAULT  # noqa: E402

SEED, N, NB, STEPS, WARM, N_SUB = 7, 20, 10, 200, 40, 2
MODES = {"off": None, "default": RECORD_DEFAULT, "default+rgp_C": RECORD_DEFAULT + ("rgp_C",)}


def rate(B, refs, rounds):
    e, _ = bench.make_engine(B, N, NB, 0, 0, 0, SEED, refs=refs)
    e.sim_steps(WARM, N_SUB, 5e-3)
    rates = {k: [] for k in MODES}
    keys = list(MODES)
    for r in range(rounds):
        for key in keys[r % 3:] + keys[:r % 3]:   # (the order rotates: every mode flies every position of a round equally often)
            fields = MODES[key]
            if fields is not None:
                e.record_start(fields=fields, capacity=STEPS)
            t0 = time.perf_counter()
            e.sim_steps(STEPS, N_SUB, 5e-3)
            rates[key].append(B * STEPS / (time.perf_counter() - t0))
            if fields is not None:
                assert e.record_info()[0] == STEPS
                e.record_stop()
    groups = e.get_groups()
    e.close()
    med = {k: float(np.median(v)) for k, v in rates.items()}
    row_bytes = {"default": 8 * (13 * 3 + 4 + 1 + 6 + 3 * NB) + 16, "default+rgp_C": 8 * (13 * 3 + 4 + 1 + 6 + 3 * NB + 3 * NB * NB) + 16}
    return {"batch": B, "N": N, "nb": NB, "groups": groups, "steps_per_call": STEPS, "rounds": rounds, "steps_per_s_median": med,
            "steps_per_s_all": rates, "cost_vs_off": {k: 1 - med[k] / med["off"] for k in ("default", "default+rgp_C")},
            "row_bytes_per_quadrotor": row_bytes, "bytes_per_period": {k: v * B for k, v in row_bytes.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batches", default="1024,8192")
    ap.add_argument("--rounds", type=int, default=6)
    args = ap.parse_args()
    batches = [int(b) for b in args.batches.split(",")]
    from mpc_quad_ros_amd import _lib
    out = {"tool": "tools/record_rate.py", "library": _lib.load().mpcq_version().decode(), "source_sha16": bench.kernel_source_sha16(),
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

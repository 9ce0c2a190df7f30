"""Cost of the sensor (mpcq_sensor_*) in the loop, on the bench workload (configs[1] shape: N = 20, RGP 10, fp64, pre-chained missions).

For B = 1024 (one group) and 8192 (two groups, split plant: the engine's automatic choices) one engine flies blocks of
`sim_steps(STEPS)`; the blocks alternate (in rotating order) between no sensor, `sensor_start(sensor_defaults(B))` -- the identity: the
flight is the same, what is added is the sensor's launch in front of every period and, at B = 1024, a plant launch per period where the
update otherwise rides at the head of the next step launch -- and a sensor with noise on every channel (a different flight: the draws,
and a controller that works against the noise).  Rate = B x STEPS / host-clock wall time of the blocking call; median over ROUNDS blocks
per mode after WARM warm-up periods.  A report, not a gate.

usage: python tools/sensor_rate.py [--out profiles/sensor_rate.json] [--batches 1024,8192] [--rounds 6]
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

SEED, N, NB, STEPS, WARM, N_SUB, DEPTH = 7, 20, 10, 200, 40, 2, 4
MODES = ("off", "identity", "noise")
NOISE = dict(sigma=dict(p=0.005, att=0.005, v=0.02, r=0.02))


def rate(B, refs, rounds):
    from mpc_quad_ros_amd.params import sensor_defaults, sensor_sample
    e, _ = bench.make_engine(B, N, NB, 0, 0, 0, SEED, refs=refs)
    e.sim_steps(WARM, N_SUB, 5e-3)
    tables = {"identity": sensor_defaults(B), "noise": sensor_sample(SEED, 0, B, **NOISE)}
    rates = {k: [] for k in MODES}
    keys = list(MODES)
    for r in range(rounds):
        for key in keys[r % 3:] + keys[:r % 3]:   # (the order rotates: every mode flies every position of a round equally often)
            if key != "off":
                e.sensor_start(tables[key], seed=SEED, depth=DEPTH)
            t0 = time.perf_counter()
            e.sim_steps(STEPS, N_SUB, 5e-3)
            rates[key].append(B * STEPS / (time.perf_counter() - t0))
            if key != "off":
                assert e.sensor_get()[2] == STEPS
                e.sensor_stop()
    groups = e.get_groups()
    e.close()
    med = {k: float(np.median(v)) for k, v in rates.items()}
    return {"batch": B, "N": N, "nb": NB, "groups": groups, "steps_per_call": STEPS, "rounds": rounds, "depth": DEPTH,
            "steps_per_s_median": med, "steps_per_s_all": rates, "cost_vs_off": {k: 1 - med[k] / med["off"] for k in ("identity", "noise")}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batches", default="1024,8192")
    ap.add_argument("--rounds", type=int, default=6)
    args = ap.parse_args()
    batches = [int(b) for b in args.batches.split(",")]
    from mpc_quad_ros_amd import _lib
    out = {"tool": "tools/sensor_rate.py", "library": _lib.load().mpcq_version().decode(), "source_sha16": bench.kernel_source_sha16(),
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

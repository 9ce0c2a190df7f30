"""What does the black box cost a period?  (needs the GPU)

sim_steps periods per second of the bench workload (N = 20, nb = 10, two plant substeps per period) at B = 1 024 (BASELINE configs[1]) and
B = 8 192, two engines from the same start state, timed alternately in one process:
  off   no black box -- the launch sequence of a library without it
  on    every quadrotor watched, the default fields, D = 64 (pre 50, post 13), rules that enable every cause with thresholds nobody
        reaches: every ring is written every period, which is what a sweep pays until its first incidents freeze
Each timed block is one sim_steps call of BLOCK periods, which returns synchronised; the host clock is around the call.

usage: python tools/blackbox_cost.py [out.json] [--off-only]     (--off-only: the `off` engine alone, for a library without the feature)
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

WARMUP, BLOCK, REPEATS, PRE, POST = 200, 200, 7, 50, 13


def measure(B, refs, modes):
    engines = {}
    for m in modes:
        e, _ = bench.make_engine(B, 20, 10, 0, 0, 0, 0, refs=refs)
        if m == "on":
            from mpc_quad_ros_amd.params import blackbox_rules
            e.blackbox_start(blackbox_rules(B, status_mask=-1, fallback=False, nonfinite=True, err_pos=1e3, speed=1e3, tilt_cos=-2.0, cost=1e300),
                             pre=PRE, post=POST)
        engines[m] = e
    for e in engines.values():
        e.sim_steps(WARMUP, 2, 5e-3)
    rates = {m: [] for m in modes}
    for _ in range(REPEATS):
        for m in modes:
            t = time.perf_counter()
            engines[m].sim_steps(BLOCK, 2, 5e-3)
            rates[m].append(BLOCK / (time.perf_counter() - t))
    out = dict(B=B, groups=engines[modes[0]].get_groups(),
               periods_per_s={m: dict(median=float(np.median(r)), min=float(min(r)), max=float(max(r)), all=[float(v) for v in r]) for m, r in rates.items()})
    out["us_per_period"] = {m: 1e6 / out["periods_per_s"][m]["median"] for m in modes}
    out["steps_per_s"] = {m: B * out["periods_per_s"][m]["median"] for m in modes}
    if "on" in modes:
        info = engines["on"].blackbox_info()
        out["fired"] = int((info["fired_period"] >= 0).sum())
        out["states_equal"] = bool(np.array_equal(engines["off"].sim_get_state()[0], engines["on"].sim_get_state()[0]))
        out["cost_us_per_period"] = out["us_per_period"]["on"] - out["us_per_period"]["off"]
    for e in engines.values():
        e.close()
    return out


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    modes = ("off",) if "--off-only" in sys.argv else ("off", "on")
    sizes = (1024, 8192)
    refs = {B: bench.workload(0, 0, B, 1000) for B in sizes}     # (forks worker processes: before this process touches the GPU)
    out = dict(block=BLOCK, repeats=REPEATS, warmup=WARMUP, D=PRE + 1 + POST, runs=[measure(B, refs[B], modes) for B in sizes])
    print(json.dumps(out))
    if args:
        with open(args[0], "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()

"""What does the exploration launch cost a period?  (needs the GPU)

sim_steps periods per second at B = 8 192 (N = 10, nb = 10, two plant substeps per period) with a mission set, three engines from the
same start state, timed alternately in one process:
  plain      the mission alone -- the launch sequence of a library without exploration
  launch     exploration started with an all-zero leg_mask: the launch runs every period and keeps the envelopes, no limit is written,
             so the flights (and every other launch) are the plain engine's -- the difference to `plain` is the launch itself
  exploring  exploration of every leg with the reference's rule numbers: other limits, so other flights; not a like-for-like figure
Each timed block is one sim_steps call of BLOCK periods, which returns synchronised; the host clock is around the call.

usage: python tools/explore_cost.py [out.json]
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mpc_quad_ros_amd.engine import Engine  # noqa: E402
from mpc_quad_ros_amd.params import EngineConfig, explore_rules, hummingbird, rgp_basis_linspace  # noqa: E402
from mpc_quad_ros_amd.trajectories import mission_legs  # noqa: E402

B, L, N_WP, TMAX, WARMUP, BLOCK, REPEATS = 8192, 12, 2, 600, 200, 200, 7


def engine(mode):
    rng = np.random.default_rng(5)
    x0 = np.tile(np.array([0, 0, 3.0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0]), (B, 1))
    x0[:, 0:3] += rng.uniform(-0.3, 0.3, (B, 3))
    wp = x0[:, None, None, 0:3] + rng.uniform(-1.0, 1.0, (B, L, N_WP, 3))
    e = Engine(EngineConfig(batch=B, N=10, T=1.0, quad=hummingbird(), nb=10, dt_pred=0.01, basis=rgp_basis_linspace(12.0, 10), theta=[1.0, 0.1, 0.1]))
    e.set_trajectories(np.repeat(x0[:, None, :], TMAX, axis=1).copy(), np.full(B, 2, np.int32))
    e.sim_reset(x0)
    e.mission_set_legs(mission_legs(B, L, 12.0, a_max=12.0), wp)
    if mode == "launch":
        e.explore_start(explore_rules(B), leg_mask=np.zeros((B, L), np.uint8))
    elif mode == "exploring":
        e.explore_start(explore_rules(B))
    return e


def main():
    modes = ("plain", "launch", "exploring")
    engines = {m: engine(m) for m in modes}
    for e in engines.values():
        e.sim_steps(WARMUP, 2, 5e-3)
    rates = {m: [] for m in modes}
    for _ in range(REPEATS):
        for m in modes:
            t = time.perf_counter()
            engines[m].sim_steps(BLOCK, 2, 5e-3)
            rates[m].append(BLOCK / (time.perf_counter() - t))
    same = bool(np.array_equal(engines["plain"].sim_get_state()[0], engines["launch"].sim_get_state()[0]))
    out = dict(B=B, block=BLOCK, repeats=REPEATS, warmup=WARMUP, groups=engines["plain"].get_groups(), plain_and_launch_states_equal=same,
               installed={m: int(engines[m].mission_get()["installed"].sum()) for m in modes},
               periods_per_s={m: dict(median=float(np.median(r)), min=float(min(r)), max=float(max(r)), all=[float(v) for v in r]) for m, r in rates.items()})
    med = {m: out["periods_per_s"][m]["median"] for m in modes}
    out["us_per_period"] = {m: 1e6 / med[m] for m in modes}
    out["launch_cost_us_per_period"] = 1e6 / med["launch"] - 1e6 / med["plain"]
    print(json.dumps(out))
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()

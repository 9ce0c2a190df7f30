"""Two builds of the library held against each other where only the HOST side of the C ABI may differ: one seeded closed-loop scenario
with every per-period feature on at once, every read-back compared bit for bit; with --time also the host-bound rate of mpcq_sim_steps.

usage: python tools/ab_libs.py --lib-a PATH --lib-b PATH [--time]

The scenario: B = 16 quadrotors (two groups of 8 with tune.groups = 2, the smallest group), N = 5, nb = 3, 8 control periods, in float64 and
in float32, driven once through sim_steps and once through step + sim_plant_period.  On at once: a recording with the drag field, a
score, a mission of one waypoint leg and one circle leg per quadrotor, an exploration over both legs, a fleet with one disturbance
window.  The flights are short (a waypoint 5 cm away, rows PLAN_DT apart, a circle of 5 cm radius) so that every quadrotor ends its hover slot
in the first period, flies its waypoint leg to the end and has its circle leg installed inside the 8 periods; library A alone has to show that
(asserted), and the comparison then covers the replan, circle, exploration and score paths of a flight's end.  Compared: engine state,
solver state, plant state and controls, every recorder field, the score table, the mission log, the exploration envelopes and limits, the
trajectories.

--time: B = 1 024, N = 20, nb = 10 (the headline shape), 200 periods of sim_steps after a warm-up, with no feature on and with all on,
the two libraries alternating, five rounds each, one process per round; per library the median rate and its spread over the rounds.

Every run of a library is a process of its own (two libmpcq in one process would share symbols)."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, N, NB, K = 16, 5, 3, 8
PLAN_DT = 0.25          # row spacing of the planned flights [s]: a flight of a second is five rows
SEED = 2027
CONTROL_DT, SIM_DT = 0.01, 5e-3
TB, TN, TNB, TK, TWARM, ROUNDS = 1024, 20, 10, 200, 40, 5
HOVER = np.array([0, 0, 3.0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0])


def make_engine(lib, batch, n, nb, prec, groups=None):
    from mpc_quad_ros_amd.engine import Engine
    from mpc_quad_ros_amd.params import PRECISION_F32, PRECISION_F64, EngineConfig, hummingbird, rgp_basis_linspace
    cfg = EngineConfig(batch=batch, N=n, T=1.0, quad=hummingbird(), nb=nb, basis=rgp_basis_linspace(12.0, nb), dt_pred=0.01,
                       precision=PRECISION_F32 if prec == "f32" else PRECISION_F64, tune=dict(groups=groups) if groups else None)
    return Engine(cfg, lib_path=lib), cfg


def features_on(e, cfg, batch, size, radius, plan_dt, tmax, capacity, seed):
    """Hover slots of two rows (everybody ends them in the first period), then: fleet, recording, score, mission, exploration."""
    from mpc_quad_ros_amd.engine import LEG_CIRCLE, LEG_WAYPOINTS
    from mpc_quad_ros_amd.params import explore_rules, fleet_sample
    from mpc_quad_ros_amd.trajectories import mission_legs
    rng = np.random.default_rng(seed)
    x0 = np.tile(HOVER, (batch, 1))
    x0[:, 0:3] += rng.uniform(-0.3, 0.3, (batch, 3))
    e.set_trajectories(np.repeat(x0[:, None, :], tmax, axis=1).copy(), np.full(batch, 2, np.int32))
    e.sim_reset(x0)
    e.fleet_set(fleet_sample(seed, 0, batch, cfg, spread=1.1, payload_max=0.05, gust_force=0.05, gust_torque=1e-3, gust_window=(2, 5)))
    e.record_start(fields=("x_odom", "x_ref", "w_odom", "x_pred_odom", "cost_solution", "drag", "rgp_mu", "solver"), capacity=capacity)
    e.score_start(3)
    wp = x0[:, None, None, 0:3] + rng.uniform(-size, size, (batch, 2, 1, 3))
    legs = mission_legs(batch, 2, 2.0, a_max=2.0, kind=np.array([LEG_WAYPOINTS, LEG_CIRCLE], np.int32), radius=radius)
    e.mission_set_legs(legs, wp, order=4, dt=plan_dt)
    e.explore_start(explore_rules(batch, step=1.0, desired=3.0, v_limit=4.0, a_limit=4.0, mode=np.arange(batch) % 2))
    return x0


def read_back(e):
    x, w = e.sim_get_state()
    traj, lens = e.get_trajectories()
    out = dict(plant_x=x, plant_w=w, traj=traj, traj_len=lens)
    out.update({f"state_{k}": v for k, v in e.get_state().items()})
    out.update({f"solver_{k}": v for k, v in e.get_solver_state().items()})
    out.update({f"rec_{k}": np.asarray(v) for k, v in e.record_get().items()})
    out.update({f"score_{k}": np.asarray(v) for k, v in e.score_get().items()})
    out.update({f"mission_{k}": v for k, v in e.mission_get().items()})
    out.update({f"explore_{k}": v for k, v in e.explore_get().items()})
    plants, period = e.fleet_get()
    out["fleet_period"] = np.asarray(period)
    out["fleet_plants"] = plants.view(np.uint8)
    return out


def child_equal(lib, path):
    """The scenario on `lib`, both precisions and both ways of driving it, into an .npz"""
    out = {}
    for prec in ("f64", "f32"):
        for drive in ("sim_steps", "step"):
            e, cfg = make_engine(lib, B, N, NB, prec, groups=2)
            assert e.get_groups() == 2
            features_on(e, cfg, B, 0.05, 0.05, PLAN_DT, 64, K, SEED)
            if drive == "sim_steps":   # (two calls: the counters carry over from call to call)
                e.sim_steps(3, e.plant_substeps(CONTROL_DT, SIM_DT), SIM_DT)
                e.sim_steps(K - 3, e.plant_substeps(CONTROL_DT, SIM_DT), SIM_DT)
            else:
                for _ in range(K):
                    x, _w = e.sim_get_state()
                    w, _xp = e.step(x)
                    e.sim_plant_period(w, CONTROL_DT, SIM_DT)
            out.update({f"{prec}_{drive}_{k}": v for k, v in read_back(e).items()})
            e.close()
    np.savez(path, **out)


def child_time(lib, path):
    """steps/s of TK periods of sim_steps at the headline shape, no feature on and all on"""
    res = {}
    for name in ("off", "on"):
        e, cfg = make_engine(lib, TB, TN, TNB, "f64")
        if name == "on":   # flights of a few hundred rows: after the first period a quadrotor flies, the side launches run every period
            features_on(e, cfg, TB, 1.5, 1.0, 0.01, 2400, TWARM + TK, SEED)
        else:
            import bench
            e.set_trajectories(*bench.workload(SEED, 0, TB, TWARM + TK + 30))
            e.sim_reset(np.tile(bench.X0, (TB, 1)))
        e.sim_steps(TWARM, 2, SIM_DT)
        e.synchronize()
        t0 = time.perf_counter()
        e.sim_steps(TK, 2, SIM_DT)
        e.synchronize()
        res[name] = TB * TK / (time.perf_counter() - t0)
        e.close()
    with open(path, "w") as fh:
        json.dump(res, fh)


def run_child(mode, lib, path):
    # (a child that faults, hangs or fails ends the tool: nothing more is started on the device behind it)
    subprocess.check_call([sys.executable, os.path.abspath(__file__), "--child", mode, "--lib-a", lib, "--out", path], timeout=600 if mode == "equal" else 240)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--lib-a", required=True)
    ap.add_argument("--lib-b")
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--child", choices=("equal", "time"), help=argparse.SUPPRESS)
    ap.add_argument("--out", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return {"equal": child_equal, "time": child_time}[a.child](a.lib_a, a.out)
    if not a.lib_b:
        ap.error("--lib-b is required")
    from mpc_quad_ros_amd.engine import REPLAN_DONE
    with tempfile.TemporaryDirectory() as tmp:
        got = {}
        for tag, lib in (("a", a.lib_a), ("b", a.lib_b)):
            run_child("equal", lib, os.path.join(tmp, tag + ".npz"))
            with np.load(os.path.join(tmp, tag + ".npz")) as z:
                got[tag] = {k: z[k] for k in z.files}
        # what the scenario is for, shown by library A alone: every quadrotor flew its waypoint leg to the end and got its circle leg
        for prec in ("f64", "f32"):
            for drive in ("sim_steps", "step"):
                p = f"{prec}_{drive}_"
                leg, code = got["a"][p + "mission_leg"], got["a"][p + "mission_leg_code"]
                assert (leg == 2).all() and (code == REPLAN_DONE).all(), f"{p}: not every quadrotor consumed both legs: leg {leg}, codes {code}"
                assert (got["a"][p + "score_flights"] >= 2).all() and got["a"][p + "rec_period"].shape == (K,), p
                assert np.isfinite(got["a"][p + "explore_leg_limits"]).all(), p
        assert sorted(got["a"]) == sorted(got["b"])
        differ = [k for k in sorted(got["a"])
                  if got["a"][k].shape != got["b"][k].shape or got["a"][k].dtype != got["b"][k].dtype or got["a"][k].tobytes() != got["b"][k].tobytes()]
        nbytes = sum(v.nbytes for v in got["a"].values())
        print(f"bit equality: {len(got['a'])} arrays, {nbytes} bytes, f64 and f32, sim_steps and step + sim_plant_period: "
              + ("all equal" if not differ else f"{len(differ)} DIFFER: {differ}"))
        rates = None
        if a.time:
            rates = {tag: {"off": [], "on": []} for tag in "ab"}
            for r in range(ROUNDS):
                for tag, lib in (("a", a.lib_a), ("b", a.lib_b)):
                    path = os.path.join(tmp, f"t_{tag}_{r}.json")
                    run_child("time", lib, path)
                    with open(path) as fh:
                        res = json.load(fh)
                    for name in ("off", "on"):
                        rates[tag][name].append(res[name])
                    print(f"round {r} lib {tag}: features off {res['off']:.0f} steps/s, on {res['on']:.0f} steps/s", flush=True)
            for name in ("off", "on"):
                for tag in "ab":
                    v = np.array(rates[tag][name])
                    print(f"sim_steps B={TB} N={TN} nb={TNB}, {TK} periods, features {name}, lib {tag}: median {np.median(v):.0f} steps/s, "
                          f"min {v.min():.0f}, max {v.max():.0f}, spread {(v.max() - v.min()) / np.median(v) * 100:.2f} %")
        print(json.dumps(dict(equal=not differ, differ=differ, rates=rates)))
        return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())

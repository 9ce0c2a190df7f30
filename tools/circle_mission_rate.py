"""Cost of a circle flight boundary: B quadrotors that all finish in the same period and all fly a circle next
(radius 10 at v_max = 12, ~1 050 rows).
 device: wall time of the one period in which the mission launch plans and installs the B circles, against the same period with an
         exhausted queue (the launch plans nothing), and the wall time of one replan_circle call;
 host:   the host path the mission replaces -- get_finished, sim_get_state, circle_trajectory x B, replace_trajectories -- which needs
         nothing newer than 0.6.1 and runs on an older build as well;
 prof:   one such period, to put under `rocprofv3 --kernel-trace --stats` (the device time of mission_kernel itself).
Usage: circle_mission_rate.py device|host|prof B"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mpc_quad_ros_amd.engine import Engine  # noqa: E402
from mpc_quad_ros_amd.params import EngineConfig, hummingbird, rgp_basis_linspace  # noqa: E402
from mpc_quad_ros_amd.trajectories import circle_trajectory  # noqa: E402

N, NB, NSUB = 20, 10, 2
RADIUS, V_MAX, DT, TMAX = 10.0, 12.0, 0.01, 1100
X0 = np.array([0, 0, 3.0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0])


def engine(B):
    cfg = EngineConfig(batch=B, N=N, T=1.0, quad=hummingbird(), nb=NB, basis=rgp_basis_linspace(12.0, NB), theta=[1.0, 0.1, 0.1], dt_pred=0.01)
    e = Engine(cfg)
    x0 = np.tile(X0, (B, 1))
    x0[:, 0:3] += np.random.default_rng(7).uniform(-0.3, 0.3, (B, 3))
    hover = np.repeat(x0[:, None, :], TMAX, axis=1)
    return e, x0, hover


def rewind(e, x0, hover):
    """Hover slots of two rows: everybody finishes in the next period."""
    e.set_trajectories(hover, np.full(e.B, 2, np.int32))
    e.sim_reset(x0)


def period(e):
    e.synchronize()
    t0 = time.perf_counter()
    e.sim_steps(1, NSUB, 5e-3)
    e.synchronize()
    return time.perf_counter() - t0


def stats(v):
    v = np.array(v[1:], float)   # (the first repetition is warm-up)
    return {"median_ms": round(1e3 * float(np.median(v)), 3), "min_ms": round(1e3 * float(v.min()), 3), "max_ms": round(1e3 * float(v.max()), 3)}


def device(B, reps=6):
    from mpc_quad_ros_amd.trajectories import mission_legs
    e, x0, hover = engine(B)
    legs = mission_legs(B, 1, V_MAX, kind="circle", radius=RADIUS)
    out = {"B": B, "rows": len(circle_trajectory("acc_dec", RADIUS, V_MAX, DT)[0]), "library": e.lib.mpcq_version().decode()}
    with_circles, idle, call = [], [], []
    for _ in range(reps):
        rewind(e, x0, hover)
        e.mission_set_legs(legs)
        with_circles.append(period(e))
        g = e.mission_get()
        assert (g["leg_code"][:, 0] == 0).all() and (e.get_finished() == 0).all()
        rewind(e, x0, hover)
        e.mission_set_legs(legs, leg0=np.ones(B, np.int32))   # queue exhausted: the launch sweeps the flags and plans nothing
        idle.append(period(e))
        e.mission_stop()
        assert (e.get_finished() == 1).all()
        t0 = time.perf_counter()
        codes = e.replan_circle(RADIUS, V_MAX)
        call.append(time.perf_counter() - t0)
        assert (codes == 0).all()
    out["period_with_circles"], out["period_idle_mission"], out["replan_circle_call"] = stats(with_circles), stats(idle), stats(call)
    out["mission_planning_ms"] = round(out["period_with_circles"]["median_ms"] - out["period_idle_mission"]["median_ms"], 3)
    print(json.dumps(out))
    e.close()


def host(B, reps=4):
    e, x0, hover = engine(B)
    out = {"B": B, "library": e.lib.mpcq_version().decode()}
    parts = {k: [] for k in ("get_finished", "sim_get_state", "circle_trajectory", "replace_trajectories", "total")}
    for _ in range(reps):
        rewind(e, x0, hover)
        e.sim_steps(1, NSUB, 5e-3)
        e.synchronize()
        t0 = time.perf_counter()
        idx = np.flatnonzero(e.get_finished())
        t1 = time.perf_counter()
        x, _ = e.sim_get_state()
        t2 = time.perf_counter()
        rows = np.zeros((len(idx), TMAX, 13))
        lens = np.zeros(len(idx), np.int32)
        for j, b in enumerate(idx):
            c, _ = circle_trajectory("acc_dec", RADIUS, V_MAX, DT, start_point=x[b, 0:3])
            rows[j, :len(c)] = c
            lens[j] = len(c)
        t3 = time.perf_counter()
        e.replace_trajectories(idx, rows, lens)
        t4 = time.perf_counter()
        assert len(idx) == B and (e.get_finished() == 0).all()
        for k, v in zip(parts, (t1 - t0, t2 - t1, t3 - t2, t4 - t3, t4 - t0)):
            parts[k].append(v)
    out.update({k: stats(v) for k, v in parts.items()})
    print(json.dumps(out))
    e.close()


def prof(B):
    from mpc_quad_ros_amd.trajectories import mission_legs
    e, x0, hover = engine(B)
    for _ in range(3):
        rewind(e, x0, hover)
        e.mission_set_legs(mission_legs(B, 1, V_MAX, kind="circle", radius=RADIUS))
        e.sim_steps(1, NSUB, 5e-3)
    print(json.dumps({"B": B, "installed": int(e.mission_get()["installed"].sum())}))
    e.close()


if __name__ == "__main__":
    {"device": device, "host": host, "prof": prof}[sys.argv[1]](int(sys.argv[2]))

"""Cost of the mission launch: steps/s of sim_steps at the bench workload shape (N = 20, nb = 10, fp64) for
(a) another build of the library, e.g. the previous release (optional), (b) this library without a mission on the bench workload,
(c) this library with a mission whose flights end, in rotating order; the periods per 1000 that quadrotors spend holding a finished
flight under the R = 10 host loop and under the mission (counted from the recorder); a plain mission run to put under
`rocprofv3 --kernel-trace --stats`.
Usage: mission_rate.py rate B [other_libmpcq.so] | holds B | prof B"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from mpc_quad_ros_amd.engine import Engine  # noqa: E402
from mpc_quad_ros_amd.params import EngineConfig, hummingbird, rgp_basis_linspace  # noqa: E402
from mpc_quad_ros_amd.trajectories import mission_waypoints  # noqa: E402

N, NB, SEED, NSUB = 20, 10, 2026, 2
X0 = np.array([0, 0, 3.0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0])


def load_other(path):
    """Another build of the library, possibly an older release without the newest entry points: every symbol it has gets its prototype."""
    import ctypes
    from mpc_quad_ros_amd import _lib
    lib = ctypes.CDLL(os.path.abspath(path))
    for name, res, args in _lib.SYMBOLS:
        fn = getattr(lib, name, None)
        if fn is not None:
            fn.restype, fn.argtypes = res, args
    _lib._cache[os.path.abspath(path)] = lib


def engine(B, lib=None):
    cfg = EngineConfig(batch=B, N=N, T=1.0, quad=hummingbird(), nb=NB, basis=rgp_basis_linspace(12.0, NB), theta=[1.0, 0.1, 0.1], dt_pred=0.01)
    return Engine(cfg, lib_path=lib)


def mission_engine(B, L, Tmax=700):
    e = engine(B)
    x0 = np.tile(X0, (B, 1))
    e.set_trajectories(np.repeat(x0[:, None, :], Tmax, axis=1), np.full(B, 2, np.int32))
    e.sim_reset(x0)
    return e, mission_waypoints(SEED, 0, B, L)


def timed(e, K):
    e.synchronize()
    t0 = time.perf_counter()
    e.sim_steps(K, NSUB, 5e-3)
    e.synchronize()
    return time.perf_counter() - t0


def rate(B, other=None, reps=6, K=200):
    refs = bench.workload(SEED, 0, B, 150 + (reps + 1) * K)
    out = {"B": B, "K": K}
    engs = {}
    if other:
        load_other(other)
    for name, lib in ((("a_other_build", other),) if other else ()) + (("b_no_mission", None),):
        e = engine(B, lib)
        e.set_trajectories(*refs)
        e.sim_reset(np.tile(X0, (B, 1)))
        e.sim_steps(150, NSUB, 5e-3)
        engs[name] = e
        out[name] = []
    e, wp = mission_engine(B, 12)
    e.mission_set(wp, 12.0, 12.0)
    e.sim_steps(150, NSUB, 5e-3)
    engs["c_mission"] = e
    out["c_mission"] = []
    for _ in range(reps):   # interleaved: a, b, c, a, b, c, ...
        for name, e in engs.items():
            out[name].append(round(B * K / timed(e, K)))
    g = engs["c_mission"].mission_get()
    out["c_installed_total"] = int(g["installed"].sum())
    out["c_periods"] = 150 + reps * K
    out["c_codes"] = {int(c): int((g["leg_code"][g["leg_period"] >= 0] == c).sum()) for c in np.unique(g["leg_code"][g["leg_period"] >= 0])}
    out["library"] = engs["c_mission"].lib.mpcq_version().decode()
    if other:
        out["other_build"] = engs["a_other_build"].lib.mpcq_version().decode()
    for name in engs:
        v = np.array(out[name][1:], float)   # (the first repetition is warm-up)
        out[name + "_median"] = float(np.median(v)); out[name + "_min"] = float(v.min()); out[name + "_max"] = float(v.max())
    print(json.dumps(out))


def holds(B, K=1000, R=10, L=16):
    out = {"B": B, "K": K, "R": R}
    for mode in ("host_loop", "mission"):
        e, wp = mission_engine(B, L)
        e.record_start(fields=("solver",), every=1, capacity=K)
        if mode == "mission":
            e.mission_set(wp, 12.0, 12.0)
            e.sim_steps(K, NSUB, 5e-3)
            installed = int(e.mission_get()["installed"].sum())
        else:
            leg, installed, ar = np.zeros(B, np.int64), 0, np.arange(B)
            for _ in range(K // R):
                e.sim_steps(R, NSUB, 5e-3)
                mask = (e.get_finished() != 0) & (leg < L)
                codes = e.replan(wp[ar, np.minimum(leg, L - 1)], 12.0, 12.0, mask=mask)
                installed += int((codes[mask] == 0).sum())
                leg[mask] += 1
        fin = e.record_get()["finished"]
        out[mode] = {"finished_rows": int(fin.sum()), "flights_installed": installed,
                     "finished_rows_per_1000_quadrotor_periods": round(1000.0 * fin.sum() / (B * K), 2),
                     "holding_per_1000": round(1000.0 * (int(fin.sum()) - installed) / (B * K), 2)}
        e.close()
    print(json.dumps(out))


def prof(B, K=300):
    e, wp = mission_engine(B, 12)
    e.mission_set(wp, 12.0, 12.0)
    e.sim_steps(150, NSUB, 5e-3)
    e.sim_steps(K, NSUB, 5e-3)
    print(json.dumps({"B": B, "installed": int(e.mission_get()["installed"].sum())}))
    e.close()


if __name__ == "__main__":
    {"rate": rate, "holds": holds, "prof": prof}[sys.argv[1]](int(sys.argv[2]), *sys.argv[3:4])

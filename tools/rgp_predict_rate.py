"""Cost of the RGP read-out (mpcq_rgp_predict / mpcq_record_predict) against the host path it replaces.

For every (B, nb) of --shapes, M = 80 query points per axis (the Visualiser's np.arange(-20, 20, 0.5)), shared grid, fp64:
  (a) host clock around Engine.rgp_predict (mean and variance), median of --rounds calls after two warm-up calls;
  (b) the path without it: Engine.get_rgp() plus the vectorised numpy restatement of tests/test_rgp_predict.py (np_predict), one CPU
      thread (the thread-count variables are set to 1 in front of the numpy import), median of --host-rounds;
  (c) with --record ROWS: a recording of ROWS periods of every quadrotor (rgp_mu, rgp_C), Engine.record_predict over all rows against
      Engine.record_get() plus the same numpy over the recorded rows.
The state of (a) / (b) is a random symmetric C and random mu loaded with set_state (the cost does not depend on the values); (c) flies
the bench workload.  The kernel's own time comes from a `rocprofv3 --kernel-trace --stats` run of this script with one shape and
--rounds 3 --host-rounds 0; bytes_floor is what the kernel must move: B x 3 x nb^2 x 8 read + 2 x B x 3 x M x 8 written.

usage: python tools/rgp_predict_rate.py [--out profiles/rgp_predict_rate.json] [--shapes 1024x10,8192x10,1024x50,8192x50] [--record 200]
"""
import argparse
import json
import os
import sys
import time

for v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
    os.environ[v] = "1"
import numpy as np  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import bench  # noqa: E402
from test_rgp_predict import np_predict, theta3  # noqa: E402

M, N, SEED = 80, 20, 7
XQ = np.tile(np.arange(-20, 20, 0.5), (3, 1))


def med(f, rounds):
    ts = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) if ts else None


def shape(B, nb, rounds, host_rounds, rec_rows, refs):
    e, cfg = bench.make_engine(B, N, nb, 0, 0, 0, SEED, refs=refs)
    rng = np.random.default_rng(SEED)
    A = rng.normal(0, 0.1, (B, 3, nb, nb))
    e.set_state(mu=rng.normal(0, 1, (B, 3, nb)), C=A + np.swapaxes(A, 2, 3))
    del A
    basis, th = np.asarray(cfg.basis), theta3(cfg.theta)
    for _ in range(2):
        e.rgp_predict(XQ)
    out = {"batch": B, "nb": nb, "M": M, "rounds": rounds,
           "bytes_floor": B * 3 * nb * nb * 8 + 2 * B * 3 * M * 8, "flop": 2 * B * 3 * M * (nb * nb + 2 * nb),
           "device_call_s": med(lambda: e.rgp_predict(XQ), rounds), "device_call_mean_only_s": med(lambda: e.rgp_predict(XQ, var=False), rounds)}
    if host_rounds:
        out["host_get_rgp_s"] = med(e.get_rgp, host_rounds)
        mu, C = e.get_rgp()
        out["host_numpy_s"] = med(lambda: np_predict(basis, th, mu, C, XQ), host_rounds)
        out["host_path_s"] = out["host_get_rgp_s"] + out["host_numpy_s"]
        out["speedup_call_vs_host_path"] = out["host_path_s"] / out["device_call_s"]
        del mu, C
    if rec_rows:
        e.reset(); e.sim_reset(np.tile(bench.X0, (B, 1)))
        e.record_start(fields=("rgp_mu", "rgp_C"), capacity=rec_rows)
        e.sim_steps(rec_rows, 2, 5e-3)
        e.record_predict(XQ, rows=(0, 1))
        r = {"rows": rec_rows, "record_predict_s": med(lambda: e.record_predict(XQ), 3), "output_bytes": 2 * B * rec_rows * 3 * M * 8,
             "recorded_bytes_not_copied": B * rec_rows * 3 * (nb + nb * nb) * 8}
        if host_rounds:
            t0 = time.perf_counter()
            rec = e.record_get()
            r["host_record_get_s"] = time.perf_counter() - t0
            t0 = time.perf_counter()
            for k in range(rec_rows):
                np_predict(basis, th, rec["rgp_mu_g_t"][:, k], rec["rgp_C_g_t"][:, k], XQ)
            r["host_numpy_s"] = time.perf_counter() - t0
            r["speedup_vs_host_path"] = (r["host_record_get_s"] + r["host_numpy_s"]) / r["record_predict_s"]
        out["recording"] = r
        e.record_stop()
    e.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", default="1024x10,8192x10,1024x50,8192x50")
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--host-rounds", type=int, default=3)
    ap.add_argument("--record", type=int, default=0)
    ap.add_argument("--record-shapes", default="1024x10")
    args = ap.parse_args()
    shapes = [tuple(int(v) for v in s.split("x")) for s in args.shapes.split(",")]
    refs = {B: bench.workload(SEED, 0, B, 1000) for B in sorted({b for b, _ in shapes})}     # (forks workers: before the GPU is touched)
    res = {"version": None, "shapes": []}
    for B, nb in shapes:
        rec = args.record if f"{B}x{nb}" in args.record_shapes.split(",") else 0
        res["shapes"].append(shape(B, nb, args.rounds, args.host_rounds, rec, refs[B]))
        print(json.dumps(res["shapes"][-1]), flush=True)
    from mpc_quad_ros_amd import _lib
    res["version"] = _lib.load().mpcq_version().decode()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

"""bench.py contract on CPU: argument surface, one JSON line with the required keys, and the N>1 launch
through torch.distributed.run (world_size 2, gloo) using the lane emulator in place of the GPU library."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REQ = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
       "vs_baseline", "dtype", "data", "config", "roofline"}


FAKE_RCCL = os.path.join(ROOT, "tests", "fake_rccl", "libfake_rccl.so")


@pytest.fixture(scope="module", autouse=True)
def build_emu():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "wave_emu")], stdout=subprocess.DEVNULL)
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "fake_rccl")], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)


def _check(line, n):
    d = json.loads(line)
    assert REQ <= set(d), REQ - set(d)
    assert d["n_gpus"] == n and d["scaling"] == "weak" and d["higher_is_better"] is True and d["vs_baseline"] is None
    assert d["dtype"] in ("f64", "f32") and d["data"] == "synthetic" and "workload" in d["config"]
    r = d["roofline"]
    assert {"bound", "achieved", "peak", "unit", "frac", "traffic"} <= set(r) and r["bound"] in ("hbm", "mfma")
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-12
    assert d["value"] > 0 and d["tracking"]["steps"] == d["config"]["global_batch"] * (d["steps"] + d["warmup"] + d["config"]["preroll_periods"])
    return d


def test_single_rank_line():
    out = subprocess.check_output([sys.executable, os.path.join(ROOT, "tests", "run_bench_emu.py"), "--steps", "2", "--warmup", "1", "--preroll", "3",
                                   "--batch", "2", "--horizon", "5", "--nb", "10", "--no-cpu-baseline", "--no-alt", "--steady", "3"], cwd=ROOT)
    lines = [ln for ln in out.decode().splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = _check(lines[0], 1)
    # the oracle-parity leg of the line (here: emulated lanes vs the oracle on the tiny workload)
    p = d["parity_on_workload"]
    assert p["quad_steps"] == 2 * 30 and p["max_rel_dev"] < 1e-7 and p["failed"] == 0
    assert d["roofline"]["traffic"] is None and "no PMC profile" in d["roofline"]["traffic_note"]
    # the representative rate next to the driver's window, and the per-rank record (one rank: min = mean = max = the line's own)
    assert d["steady_state"]["steps"] == 3 and d["steady_state"]["value"] > 0
    pr = d["per_rank"]
    assert pr["steps_per_s"]["min"] == pr["steps_per_s"]["max"] and len(pr["ranks"]) == 1 and 0.5 < d["efficiency_vs_best_rank"] <= 1.0 + 1e-9
    # the latency floor of a launch: chain latencies from profiles/r5_chain_floor.json x the work counters read back after every launch
    lr = d["latency_roofline"]
    assert lr["launches"] == 20 and lr["floor_ms"] > 0 and abs(lr["frac"] - lr["floor_ms"] / lr["achieved_ms"]) < 1e-9 and lr["slowest_quad_factorisations_mean"] >= 1


def test_two_ranks_under_torchrun():
    import socket
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "tests", "run_bench_emu.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--preroll", "3",
           "--batch", "2", "--horizon", "5", "--nb", "10", "--no-strict-rccl"]      # (no RCCL without GPUs: the statistic goes over the host group, and the line says so)
    out = subprocess.check_output(cmd, cwd=ROOT, stderr=subprocess.STDOUT, timeout=600)
    lines = [ln for ln in out.decode().splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.decode()[-2000:]
    d = _check(lines[0], 2)
    assert d["config"]["global_batch"] == 4 and d["config"]["parallelism"] == "shard2"
    assert "cpu_baseline" not in d and "alt_precision" not in d and "steady_state" not in d        # rank-0, N=1 only
    # every rank's own clock, gathered over the host group: the line carries min / mean / max and the efficiency against the best rank
    pr = d["per_rank"]
    assert len(pr["ranks"]) == 2 and {"ms_per_step", "kernel_avg_ms", "steps_per_s"} <= set(pr["ranks"][0])
    for k in ("ms_per_step", "kernel_avg_ms", "steps_per_s"):
        assert pr[k]["min"] <= pr[k]["mean"] <= pr[k]["max"]
    assert abs(d["efficiency_vs_best_rank"] - d["value"] / (2 * pr["steps_per_s"]["max"])) < 1e-12 and d["efficiency_vs_best_rank"] <= 1.0 + 1e-9
    assert d["config"]["batch_per_gpu"] == 2 and d["config"]["rccl_ok"] is False and "gloo" in d["config"]["stats_reduce"]


def test_two_ranks_strict_rccl_is_the_default():
    """Under WORLD_SIZE > 1 a reduction that did not go through RCCL fails the run unless --no-strict-rccl says otherwise."""
    import socket
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "tests", "run_bench_emu.py"), "--gpus", "2", "--steps", "1", "--warmup", "1", "--preroll", "1",
           "--batch", "1", "--horizon", "5", "--nb", "0"]
    r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert r.returncode != 0
    lines = [ln for ln in r.stdout.decode().splitlines() if ln.startswith("{")]
    assert len(lines) == 1 and json.loads(lines[0])["config"]["rccl_ok"] is False      # the line is still printed, and says which reduction ran


def test_eight_ranks_reduce_both_statistics_through_the_rccl_branch():
    """Dry run of the driver's 8-GPU launch (python -m torch.distributed.run --nproc-per-node 8 bench.py --gpus 8): eight ranks on the
    lane emulator, with the RCCL branch of libmpcq ACTIVE -- MPCQ_RCCL_LIB points the library at a test-only stand-in that reduces over
    shared memory (tests/fake_rccl) -- and strict mode on (the default): unique id from rank 0, one communicator per rank, the configs[1]
    headline reduced through it, the configs[3] swarm leg (its own engine, here 2 quadrotors per rank) reduced through the SAME
    communicator (mpcq_comm_share), both statistics complete, the line self-consistent over 8 ranks."""
    import socket
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "8", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "tests", "run_bench_emu.py"), "--gpus", "8", "--steps", "2", "--warmup", "1", "--preroll", "2",
           "--batch", "1", "--horizon", "5", "--nb", "0", "--swarm-per-rank", "2"]
    env = dict(os.environ, MPCQ_RCCL_LIB=FAKE_RCCL, OMP_NUM_THREADS="1")
    r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=1500, env=env)
    assert r.returncode == 0, r.stdout.decode()[-3000:]           # strict mode: a reduction that fell back to the host group would exit non-zero
    lines = [ln for ln in r.stdout.decode().splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout.decode()[-3000:]
    d = _check(lines[0], 8)
    assert d["config"]["global_batch"] == 8 and d["config"]["batch_per_gpu"] == 1 and d["config"]["parallelism"] == "shard8"
    assert d["config"]["stats_reduce"] == "rccl" and d["config"]["rccl_ok"] is True
    pr = d["per_rank"]
    assert len(pr["ranks"]) == 8
    assert abs(d["efficiency_vs_best_rank"] - d["value"] / (8 * pr["steps_per_s"]["max"])) < 1e-12 and 0 < d["efficiency_vs_best_rank"] <= 1.0 + 1e-9
    # every rank reports how long its host-side generation of the references took under 8 concurrent ranks (round-5 verdict, item 9): the
    # driver's budget is minutes; here (tiny shapes, eight processes on the CPUs of this container) seconds
    assert all(0 <= r["host_generation_s"] < 120 for r in pr["ranks"])
    # the swarm leg: 2 quadrotors on each of 8 ranks, its statistic over the same communicator
    sw = d["swarm"]
    assert sw["n_gpus"] == 8 and sw["global_batch"] == 16 and sw["stats_reduce"] == "rccl"
    assert len(sw["per_rank"]["ranks"]) == 8 and 0 < sw["efficiency_vs_best_rank"] <= 1.0 + 1e-9
    assert sw["tracking_steps"] == 16 * (2 + 5 + 20)              # every rank's (pre-roll + warm-up + timed) periods arrived in the sum
    assert d["tracking"]["steps"] == 8 * (2 + 1 + 2)


def _dump_run(tmp, name, steps, warmup):
    d = os.path.join(tmp, name)
    out = subprocess.check_output([sys.executable, os.path.join(ROOT, "tests", "run_bench_emu.py"), "--steps", str(steps), "--warmup", str(warmup),
                                   "--preroll", "3", "--batch", "2", "--horizon", "5", "--nb", "10", "--no-cpu-baseline", "--no-alt", "--no-parity",
                                   "--steady", "0", "--dump-outputs", d], cwd=ROOT)
    lines = [ln for ln in out.decode().splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    line = _check(lines[0], 1)
    assert line["steps"] == steps and line["dump_outputs"]["quads"] == 2 and line["dump_outputs"]["bytes"] <= 64 * 10**6
    files = sorted(os.listdir(d))
    assert files == line["dump_outputs"]["files"]
    return {f[:-4]: np.load(os.path.join(d, f)) for f in files}


def test_dump_outputs_are_reproducible_and_end_at_the_last_timed_step(tmp_path):
    """--dump-outputs DIR: the arrays the timed path left behind, float64, bit for bit the same from run to run with the same
    arguments; the same periods split differently between warm-up and timed steps end in the same state, one timed step more does not."""
    a = _dump_run(str(tmp_path), "a", 2, 1)
    assert a["plant_state"].shape == (2, 13) and a["control"].shape == (2, 4) and a["pred_states"].shape == (2, 6, 13)
    assert a["pred_inputs"].shape == (2, 5, 4) and a["rgp_C"].shape == (2, 3, 10, 10) and np.array_equal(a["quad_index"], [0, 1])
    assert all(v.dtype == np.float64 for v in a.values()) and np.isfinite(a["plant_state"]).all()
    b = _dump_run(str(tmp_path), "b", 2, 1)
    c = _dump_run(str(tmp_path), "c", 1, 2)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
        assert np.array_equal(a[k], c[k]), k
    d = _dump_run(str(tmp_path), "d", 3, 1)
    assert not np.array_equal(a["plant_state"], d["plant_state"])


def test_dump_outputs_sample_stays_within_64_mb(tmp_path):
    """The largest BASELINE shape (8192 quadrotors, N = 50, 50 basis points) is ~0.5 GB of outputs: a fixed seeded sample of the
    quadrotors, the same rows in every file, under 64 MB in all (a stand-in engine: no device needed)."""
    import bench

    class Stub:
        def __init__(self, B, N, nb):
            self.B, self.N, self.nb = B, N, nb
            self.base = np.arange(B, dtype=np.float64)

        def sim_get_state(self):
            return np.repeat(self.base[:, None], 13, 1), np.repeat(self.base[:, None], 4, 1)

        def get_state(self):
            B, N, nb = self.B, self.N, self.nb
            col = lambda *s: np.broadcast_to(self.base.reshape((B,) + (1,) * len(s)), (B,) + s).copy()
            return dict(X=col(N + 1, 13), U=col(N, 4), mu=col(3, nb), C=col(3, nb, nb), x_pred_prev=col(13),
                        has_prev=np.ones(B, np.int32), idx=np.zeros(B, np.int32))

        def get_status(self):
            return self.base.astype(np.int32)

        def get_solver_state(self):
            return {"stats": np.repeat(self.base[:, None], 4, 1)}

    r = bench.dump_outputs(Stub(8192, 50, 50), str(tmp_path / "big"), 8192, bench.DUMP_BYTES)
    assert r["bytes"] <= 64 * 10**6 and 0 < r["quads"] < 8192
    assert sum(os.path.getsize(tmp_path / "big" / f) for f in os.listdir(tmp_path / "big")) == r["bytes"]
    idx = np.load(tmp_path / "big" / "quad_index.npy")
    assert len(idx) == r["quads"] and (np.diff(idx) > 0).all()
    for f in r["files"]:
        a = np.load(tmp_path / "big" / f)
        assert a.dtype == np.float64 and len(a) == r["quads"]
        if f != "quad_index.npy":
            assert np.array_equal(a.reshape(len(a), -1)[:, 0], idx - 8192), f     # every file holds the rows of the same quadrotors
    bench.dump_outputs(Stub(8192, 50, 50), str(tmp_path / "again"), 8192, bench.DUMP_BYTES)
    assert np.array_equal(np.load(tmp_path / "again" / "quad_index.npy"), idx)  # a fixed sample
    small = bench.dump_outputs(Stub(1024, 20, 10), str(tmp_path / "small"), 0, bench.DUMP_BYTES)
    assert small["quads"] == 1024                                                # the default workload is written whole

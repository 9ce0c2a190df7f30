"""The flight recorder (mpcq_record_*): per-period rows of selected quadrotors written on the device during closed-loop runs.  The same
cases run on the lane emulator (CPU, small batches) and on the MI355X (-m gpu, the product library, large batches).  Yardsticks: the
engine's own per-period read-back (bit for bit), the fp64 oracle's compute_a_drag and the reference's logged run."""
import os
import subprocess

import numpy as np
import pytest

from helpers import config_for_log, load_golden, visualiser_summaries
from mpc_quad_ros_amd import _lib
from mpc_quad_ros_amd.engine import RECORD_FIELDS, Engine
from mpc_quad_ros_amd.logger import REFERENCE_KEYS, SwarmLogger
from mpc_quad_ros_amd.params import EngineConfig, hummingbird, rgp_basis_linspace
from oracle.oracle import OracleEngine, compute_a_drag

EMU_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "wave_emu")
EMU = os.path.join(EMU_DIR, "libmpcq_emu.so")
HOVER = np.array([0, 0, 3.0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0])
MPCQ_ERR_INVALID, MPCQ_ERR_STATE = -1, -3
ALL = tuple(RECORD_FIELDS)
SNAP_KEYS = ("x_odom", "x_ref", "w_odom", "x_pred_odom", "cost_solution", "v_body", "a_drag", "rgp_mu_g_t", "rgp_C_g_t", "status", "qp_iter",
             "idx", "finished", "period")


@pytest.fixture(scope="module")
def emu():
    subprocess.check_call(["make", "-C", EMU_DIR], stdout=subprocess.DEVNULL)
    return EMU


def config(B, N=10, nb=10, **kw):
    extra = dict(basis=rgp_basis_linspace(12.0, nb), theta=[1.0, 0.1, 0.1]) if nb else {}
    return EngineConfig(batch=B, N=N, T=1.0, quad=hummingbird(), nb=nb, dt_pred=0.01, **extra, **kw)


def ramp_slots(B, length=30, seed=0):
    """Every quadrotor on a slow straight flight of `length` rows from a start near hover: cursors run past the end within
    `length` periods and the finished flags flip."""
    rng = np.random.default_rng(seed)
    x0 = np.tile(HOVER, (B, 1))
    x0[:, 0:3] += rng.uniform(-0.3, 0.3, (B, 3))
    traj = np.repeat(x0[:, None, :], length, axis=1).copy()
    traj[:, :, 0] += 0.01 * np.arange(length)[None, :]
    traj[:, :, 7] = 0.1
    return x0, traj, np.full(B, length, np.int32)


def new_engine(lib, B, seed=0, length=30, **kw):
    e = Engine(config(B, **kw), lib_path=lib)
    x0, traj, lens = ramp_slots(B, length, seed)
    e.set_trajectories(traj, lens)
    e.sim_reset(x0)
    return e


def expect_rc(rc, fn, *args, **kw):
    with pytest.raises(_lib.MpcqError, match=f"mpcq error {rc}:"):
        fn(*args, **kw)


def same(a, b, keys=SNAP_KEYS):
    for k in keys:
        if k in a or k in b:
            assert np.array_equal(a[k], b[k], equal_nan=True), k


def snapshot(e):
    x, w = e.sim_get_state()
    t, ln = e.get_trajectories()
    return dict(x=x, w=w, traj=t, len=ln, stats=e.get_tracking_stats(), **{f"st_{k}": v for k, v in e.get_state().items()},
                **{f"sv_{k}": v for k, v in e.get_solver_state().items()})


# ------------------------------------------------------------------ cases (engine library, batch)
def case_readback(lib, B, K, n_sub=2):
    """A recording of one sim_steps(K) call equals, bit for bit, what K calls of sim_steps(1) leave readable after each period."""
    a = new_engine(lib, B)
    a.record_start(fields=ALL, capacity=K)
    a.sim_steps(K, n_sub, 5e-3)
    rec = a.record_get()
    assert a.record_info() == (K, 0, K)
    b = new_engine(lib, B)
    per = {k: [] for k in ("x_odom", "x_ref", "w_odom", "x_pred_odom", "cost_solution", "rgp_mu_g_t", "rgp_C_g_t", "status", "qp_iter", "idx",
                           "finished")}
    for _ in range(K):
        per["x_odom"].append(b.sim_get_state()[0])
        per["x_ref"].append(b.get_reference_chunk()[:, 0])
        b.sim_steps(1, n_sub, 5e-3)
        st = b.get_state()
        per["w_odom"].append(b.sim_get_state()[1]); per["cost_solution"].append(b.get_cost())
        per["x_pred_odom"].append(st["x_pred_prev"]); per["idx"].append(st["idx"] - 1)
        per["rgp_mu_g_t"].append(st["mu"]); per["rgp_C_g_t"].append(st["C"])
        per["status"].append(b.get_status()); per["qp_iter"].append(b.get_qp_iter()); per["finished"].append(b.get_finished())
    for k, v in per.items():
        assert np.array_equal(rec[k], np.swapaxes(np.stack(v), 0, 1)), k
    assert np.array_equal(rec["period"], np.arange(K)) and np.array_equal(rec["quads"], np.arange(B)) and rec["dropped"] == 0
    assert rec["finished"][:, -1].all() and not rec["finished"][:, 0].any()      # the cursors ran past the end
    assert (rec["idx"][:, -1] >= 29).all()
    for j in range(B):
        for k in range(K):
            xpm1 = rec["x_pred_odom"][j, k - 1] if k else rec["x_odom"][j, 0]
            vb, ad = compute_a_drag(rec["x_odom"][j, k], xpm1, 0.01)
            assert np.abs(rec["v_body"][j, k] - vb).max() <= 1e-14 and np.abs(rec["a_drag"][j, k] - ad).max() <= 1e-12, (j, k)
    same(snapshot(a), snapshot(b), snapshot(a).keys())
    a.close(); b.close()
    return rec


def continuous(lib, B, K, record, replan_every=0, quads=None, fields=ALL, tune=None, N=10, seed=1):
    """sim_steps in chunks, with replans of the finished quadrotors between them; returns (engine snapshot, recording or None)."""
    e = new_engine(lib, B, N=N, tune=tune, seed=seed)
    rng = np.random.default_rng(seed)
    if record:
        e.record_start(quads=quads, fields=fields, capacity=K)
    done = 0
    while done < K:
        n = min(5, K - done)
        e.sim_steps(n, 2, 5e-3)
        done += n
        if replan_every:
            x, _ = e.sim_get_state()
            e.replan(x[:, None, 0:3] + rng.uniform(-0.5, 0.5, (B, 1, 3)), 12.0, 12.0)
    rec = e.record_get() if record else None
    out = snapshot(e)
    e.close()
    return out, rec


def case_no_perturbation(lib, B, K, **kw):
    a, rec = continuous(lib, B, K, True, replan_every=1, **kw)
    b, _ = continuous(lib, B, K, False, replan_every=1, **kw)
    same(a, b, a.keys())
    assert rec["x_odom"].shape[1] == K
    return rec


def case_selection_order(lib, B, K, quads, **kw):
    """A selection in the caller's (unsorted) order returns the matching rows of the full recording."""
    _, full = continuous(lib, B, K, True, **kw)
    _, sub = continuous(lib, B, K, True, quads=quads, **kw)
    assert np.array_equal(sub["quads"], quads)
    for k in SNAP_KEYS:
        if k == "period":
            assert np.array_equal(sub[k], full[k])
        else:
            assert np.array_equal(sub[k], full[k][quads]), k
    return full


def case_decimation(lib, B):
    ref = new_engine(lib, B)
    ref.record_start(capacity=30)
    ref.sim_steps(30, 2, 5e-3)
    full = ref.record_get()
    ref.close()
    e = new_engine(lib, B)
    e.record_start(every=3, capacity=5)
    e.sim_steps(8, 2, 5e-3)
    e.sim_steps(12, 2, 5e-3)
    r = e.record_get()
    assert np.array_equal(r["period"], [0, 3, 6, 9, 12]) and r["dropped"] == 2 and e.record_info() == (5, 2, 20)
    keys = [k for k in SNAP_KEYS if k != "period" and k in r]
    assert len(keys) == 12
    for k in keys:
        assert np.array_equal(r[k], full[k][:, r["period"]]), k
    e.record_clear()
    assert e.record_info() == (0, 0, 20)
    e.sim_steps(10, 2, 5e-3)
    r = e.record_get()
    assert np.array_equal(r["period"], [21, 24, 27]) and r["dropped"] == 0
    for k in keys:
        assert np.array_equal(r[k], full[k][:, r["period"]]), k
    e.close()


def case_golden_log(lib, K):
    """The reference's own run through mpcq_step, teacher-forced as tests/test_oracle_golden.py does, recorded."""
    g = load_golden("log_traj0_v10_a10_gp2.npz")
    e = Engine(config_for_log(g), lib_path=lib)
    e.set_trajectories(g["x_ref"][None])
    e.record_start(capacity=K)
    for k in range(K):
        if k > 0:
            e.set_state(x_pred_prev=g["x_pred_odom"][k - 1][None])
        e.step(g["x_odom"][k][None])
    rec = e.record_get()
    assert np.array_equal(rec["x_odom"][0], g["x_odom"][:K])
    assert np.array_equal(rec["x_ref"][0], g["x_ref"][:K])
    assert np.abs(rec["v_body"][0] - g["v_body"][:K]).max() < 1e-14 and np.abs(rec["a_drag"][0] - g["a_drag"][:K]).max() < 1e-12
    scale = np.maximum(1.0, np.abs(g["rgp_mu"][:K]).max(axis=(1, 2)))
    assert (np.abs(rec["rgp_mu_g_t"][0] - g["rgp_mu"][:K]).max(axis=(1, 2)) / scale).max() < 1e-10
    assert np.abs(rec["w_odom"][0] - g["w_odom"][:K]).max() < 5e-6            # tests/test_oracle_golden.py LOGS_GP
    # the recorded prediction is the nominal model's from the recorded measurement and control (as the log's is from its own)
    cfg = config_for_log(g, batch=K)
    xp = OracleEngine(cfg).predict_nominal(rec["x_odom"][0], rec["w_odom"][0], cfg.dt_pred)
    assert np.abs(rec["x_pred_odom"][0] - xp).max() < 1e-14
    assert np.abs(rec["x_pred_odom"][0] - g["x_pred_odom"][:K]).max() < 1e-5
    assert (rec["status"][0] == 0).all() and np.array_equal(rec["idx"][0], np.arange(K))
    # ... into the reference's log layout and its analysis
    import tempfile
    lg = SwarmLogger.from_recording(e, rec, control_dt=0.1, t_cpu=1e-3)
    log = lg.quad_log(0)
    assert tuple(log) == REFERENCE_KEYS
    assert log["v_body"].shape == (K, 3, 1) and log["a_drag"].shape == (K, 3, 1) and log["t_cpu"].shape == (K, 1)
    assert log["rgp_basis_vectors"].shape == (K, 3, e.nb) and log["rgp_theta"].shape == (K, 3, 3)
    assert np.allclose(log["t_odom"], 0.1 * np.arange(K), rtol=0, atol=1e-15)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "log.pkl")
        lg.save(path, 0)
        s = visualiser_summaries(path)
    stats = e.get_tracking_stats()
    assert abs(s["rms_total"] - np.sqrt(stats[0] / (3 * stats[2]))) <= 1e-12 * s["rms_total"]
    own = visualiser_summaries(dict(x_odom=g["x_odom"][:K], x_ref=g["x_ref"][:K], t_cpu=np.zeros((K, 1))))
    assert np.array_equal(s["rms_pos_ref"], own["rms_pos_ref"])
    assert abs(s["avg_cpu"] - 1e-3) < 1e-18 and np.allclose(lg.rms_position_error()[0], s["rms_total"], rtol=1e-12)
    e.close()


def case_f32(lib, B, K):
    """MPCQ_PRECISION_F32: mu, C and cost recorded equal, bit for bit, what get_rgp / get_cost read after each period."""
    a = new_engine(lib, B, precision=1)
    a.record_start(fields=("rgp_mu", "rgp_C", "cost_solution"), capacity=K)
    a.sim_steps(K, 2, 5e-3)
    rec = a.record_get()
    assert set(rec) == {"rgp_mu_g_t", "rgp_C_g_t", "cost_solution", "period", "quads", "dropped"}
    b = new_engine(lib, B, precision=1)
    mus, Cs, costs = [], [], []
    for _ in range(K):
        b.sim_steps(1, 2, 5e-3)
        mu, C = b.get_rgp()
        mus.append(mu); Cs.append(C); costs.append(b.get_cost())
    assert np.array_equal(rec["rgp_mu_g_t"], np.swapaxes(np.stack(mus), 0, 1))
    assert np.array_equal(rec["rgp_C_g_t"], np.swapaxes(np.stack(Cs), 0, 1))
    assert np.array_equal(rec["cost_solution"], np.swapaxes(np.stack(costs), 0, 1))
    assert np.abs(rec["rgp_mu_g_t"]).max() > 0
    a.close(); b.close()


def case_errors(lib, B):
    e = new_engine(lib, B)
    L = e.lib
    q = np.array([0, 1], np.int32)
    assert L.mpcq_record_start(e.h, _lib.i(q), 0, 1, 1, 10) == MPCQ_ERR_INVALID                  # count <= 0 with quads
    assert L.mpcq_record_start(e.h, _lib.i(q), -1, 1, 1, 10) == MPCQ_ERR_INVALID
    for quads in ([B], [-1], [1, 1]):
        expect_rc(MPCQ_ERR_INVALID, e.record_start, quads=quads)
    for fields in (0, 512, 1 | 1024):
        assert L.mpcq_record_start(e.h, None, 0, fields, 1, 10) == MPCQ_ERR_INVALID
    expect_rc(MPCQ_ERR_INVALID, e.record_start, every=0)
    expect_rc(MPCQ_ERR_INVALID, e.record_start, capacity=0)
    n0 = Engine(config(B, nb=0), lib_path=lib)
    for f in ("rgp_mu", "rgp_C"):
        expect_rc(MPCQ_ERR_INVALID, n0.record_start, fields=("x_odom", f))
    n0.record_start()                                       # the default drops the RGP fields without an RGP
    n0.record_stop()
    n0.close()
    # nothing active
    expect_rc(MPCQ_ERR_STATE, e.record_get)
    expect_rc(MPCQ_ERR_STATE, e.record_info)
    expect_rc(MPCQ_ERR_STATE, e.record_clear)
    expect_rc(MPCQ_ERR_STATE, e.record_stop)
    out = np.zeros(64)
    assert L.mpcq_record_get_solver(e.h, _lib.i(np.zeros(64, np.int32))) == MPCQ_ERR_STATE
    assert L.mpcq_record_get_periods(e.h, _lib.l(np.zeros(4, np.int64))) == MPCQ_ERR_STATE
    e.record_start(fields=("x_odom", "w_odom", "solver"))
    expect_rc(MPCQ_ERR_STATE, e.record_start)
    for field in (2, 256, 1 | 4, 0, 512):                   # not recorded, the int field, two bits, none, unknown
        assert L.mpcq_record_get(e.h, field, _lib.d(out)) == MPCQ_ERR_INVALID, field
    expect_rc(MPCQ_ERR_STATE, e.sim_run, 3, 2)
    e.record_stop()
    e.close()
    # after record_stop, sim_run gives what an engine that never recorded gives
    a, b = new_engine(lib, B), new_engine(lib, B)
    a.record_start()
    a.record_stop()
    a.sim_run(6, 2); b.sim_run(6, 2)
    same(snapshot(a), snapshot(b), snapshot(a).keys())
    a.close(); b.close()


# ------------------------------------------------------------------ lane emulator (CPU)
def test_emu_recording_equals_per_period_readback(emu):
    case_readback(emu, 6, 30)


def test_emu_recording_does_not_perturb_the_flight(emu):
    case_no_perturbation(emu, 6, 12)


def test_emu_groups_and_selection_order(emu):
    """Two groups of 8 (mpcq_sim_steps launches per group): the recording of one group equals that of the whole batch, and a selection
    across the group boundary comes back in the caller's order."""
    a, ra = continuous(emu, 16, 6, True, tune=dict(groups=1))
    b, rb = continuous(emu, 16, 6, True, tune=dict(groups=2))
    same(a, b, a.keys()); same(ra, rb)
    case_selection_order(emu, 16, 6, np.array([9, 2, 15, 7, 8]), tune=dict(groups=2))


def test_emu_decimation_capacity_clear(emu):
    case_decimation(emu, 5)


def test_emu_reference_log_through_step(emu):
    case_golden_log(emu, 12)


def test_emu_f32_rgp_and_cost(emu):
    case_f32(emu, 4, 8)


def test_emu_errors(emu):
    case_errors(emu, 4)


# ------------------------------------------------------------------ MI355X
gpu = pytest.mark.gpu


@gpu
def test_gpu_recording_equals_per_period_readback():
    case_readback(None, 1024, 100)


@gpu
def test_gpu_recording_does_not_perturb_the_flight_b8192(monkeypatch):
    monkeypatch.setenv("MPCQ_TUNING", "1")
    monkeypatch.setenv("MPCQ_SPLIT_PLANT", "1")
    rec = case_no_perturbation(None, 8192, 40, N=20, tune=dict(groups=2))
    assert rec["x_odom"].shape == (8192, 40, 13)


@gpu
def test_gpu_groups_bit_identical():
    a, ra = continuous(None, 1024, 30, True, replan_every=1, tune=dict(groups=1))
    b, rb = continuous(None, 1024, 30, True, replan_every=1, tune=dict(groups=4))
    same(a, b, a.keys()); same(ra, rb)


@gpu
def test_gpu_split_plant_bit_identical(monkeypatch):
    monkeypatch.setenv("MPCQ_TUNING", "1")
    monkeypatch.setenv("MPCQ_SPLIT_PLANT", "0")
    a, ra = continuous(None, 1024, 30, True, replan_every=1)
    monkeypatch.setenv("MPCQ_SPLIT_PLANT", "1")
    b, rb = continuous(None, 1024, 30, True, replan_every=1)
    same(a, b, a.keys()); same(ra, rb)


@gpu
def test_gpu_selection_across_groups_in_caller_order():
    quads = np.array([1000, 3, 256, 255, 767, 768, 512, 511, 0, 1023])     # both sides of every boundary of four groups of 256
    case_selection_order(None, 1024, 20, quads, tune=dict(groups=4))


@gpu
def test_gpu_decimation_capacity_clear():
    case_decimation(None, 256)


@gpu
def test_gpu_reference_log_through_step():
    case_golden_log(None, 100)


@gpu
def test_gpu_f32_rgp_and_cost():
    case_f32(None, 1024, 20)


@gpu
def test_gpu_errors():
    case_errors(None, 1024)


class _Hip:
    """Raw float64 device buffers for the device-pointer entry point."""
    def __init__(self):
        import ctypes
        self.ct = ctypes
        self.lib = ctypes.CDLL("libamdhip64.so")
        self.lib.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
        self.lib.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
        self.lib.hipFree.argtypes = [ctypes.c_void_p]

    def alloc(self, nbytes):
        p = self.ct.c_void_p()
        assert self.lib.hipMalloc(self.ct.byref(p), nbytes) == 0
        return p.value

    def h2d(self, dst, a):
        a = np.ascontiguousarray(a)
        assert self.lib.hipMemcpy(self.ct.c_void_p(dst), a.ctypes.data_as(self.ct.c_void_p), a.nbytes, 1) == 0

    def d2h(self, a, src):
        assert self.lib.hipMemcpy(a.ctypes.data_as(self.ct.c_void_p), self.ct.c_void_p(src), a.nbytes, 2) == 0

    def free(self, p):
        self.lib.hipFree(self.ct.c_void_p(p))


@gpu
def test_gpu_device_pointer_path():
    """step_device_async records the caller's device measurement and the control it wrote to the caller's buffer."""
    hip = _Hip()
    B, K = 512, 5
    e = new_engine(None, B)
    e.record_start(fields=("x_odom", "w_odom"), capacity=K)
    x0, _, _ = ramp_slots(B)
    dx, dw = hip.alloc(B * 13 * 8), hip.alloc(B * 4 * 8)
    xs, ws = [], []
    for k in range(K):
        x = x0 + 0.01 * k
        hip.h2d(dx, x)
        e.step_device_async(dx, dw)
        e.synchronize()
        w = np.zeros((B, 4))
        hip.d2h(w, dw)
        xs.append(x); ws.append(w)
    rec = e.record_get()
    assert np.array_equal(rec["x_odom"], np.swapaxes(np.stack(xs), 0, 1))
    assert np.array_equal(rec["w_odom"], np.swapaxes(np.stack(ws), 0, 1))
    e.record_stop()
    e.close()
    hip.free(dx); hip.free(dw)

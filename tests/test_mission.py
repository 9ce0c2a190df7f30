"""Device missions: mpcq_mission_set / mpcq_mission_get / mpcq_mission_stop -- a queue of upcoming flights per quadrotor and a launch
behind every period that installs the next one for whoever just finished.  The same cases run on the lane emulator (CPU, small
batches) and on the MI355X (-m gpu, the product library).

The yardstick is the host loop that exists without missions, per period: sim_steps(1) (or step(x)); fin = get_finished();
mask = fin & (leg < L); replan(wp[b, leg[b]], mask = mask) (or replan_nonlinear); leg[mask] += 1.  A mission is the same arithmetic in
the same order, so every comparison against it is bit for bit."""
import os
import subprocess

import numpy as np
import pytest

from mpc_quad_ros_amd import _lib
from mpc_quad_ros_amd.engine import REPLAN_BAD_INPUT, REPLAN_DONE, REPLAN_SKIPPED, REPLAN_TOO_LONG, Engine
from mpc_quad_ros_amd.params import EngineConfig, hummingbird, rgp_basis_linspace
from mpc_quad_ros_amd.trajectories import flight_waypoints, mission_waypoints

EMU_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "wave_emu")
EMU = os.path.join(EMU_DIR, "libmpcq_emu.so")
HOVER = np.array([0, 0, 3.0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0])
MPCQ_ERR_INVALID, MPCQ_ERR_STATE = -1, -3
V_MAX = A_MAX = 12.0
DT = 0.01


@pytest.fixture(scope="module")
def emu():
    subprocess.check_call(["make", "-C", EMU_DIR], stdout=subprocess.DEVNULL)
    return EMU


def config(B, N=10, nb=10, **kw):
    extra = dict(basis=rgp_basis_linspace(12.0, nb), theta=[1.0, 0.1, 0.1]) if nb else {}
    return EngineConfig(batch=B, N=N, T=1.0, quad=hummingbird(), nb=nb, dt_pred=0.01, **extra, **kw)


def expect_rc(rc, fn, *args, **kw):
    with pytest.raises(_lib.MpcqError, match=f"mpcq error {rc}:"):
        fn(*args, **kw)


def workload(B, L, n_wp, size, seed, Tmax=400):
    """Start points, hover slots of two rows (everybody finishes in the first period) and a queue of L legs of n_wp waypoints within
    +-size of the start point."""
    rng = np.random.default_rng(seed)
    x0 = np.tile(HOVER, (B, 1))
    x0[:, 0:3] += rng.uniform(-0.3, 0.3, (B, 3))
    traj = np.repeat(x0[:, None, :], Tmax, axis=1).copy()
    wp = x0[:, None, None, 0:3] + rng.uniform(-size, size, (B, L, n_wp, 3))
    return x0, traj, np.full(B, 2, np.int32), wp


def start_engine(lib, B, x0, traj, lens, **cfg):
    e = Engine(config(B, **cfg), lib_path=lib)
    e.set_trajectories(traj, lens)
    e.sim_reset(x0)
    return e


def snapshot(e):
    x, w = e.sim_get_state()
    t, ln = e.get_trajectories()
    return dict(x=x, w=w, traj=t, len=ln, **{f"st_{k}": v for k, v in e.get_state().items()},
                **{f"sv_{k}": v for k, v in e.get_solver_state().items()})


def assert_same(a, b, keys=None):
    for k in keys or a:
        assert np.array_equal(a[k], b[k], equal_nan=True), k


def plan(e, wp_now, mask, start, order, nonlinear, opts):
    if nonlinear:
        return e.replan_nonlinear(wp_now, V_MAX, A_MAX, DT, order, start=start, mask=mask, opts=opts)[0]
    return e.replan(wp_now, V_MAX, A_MAX, DT, order, start=start, mask=mask)


def host_loop(e, wp, K, order=4, nonlinear=False, opts=None, x_meas=None, leg=None, log=None, k0=0):
    """The yardstick.  x_meas: None = the on-device plant (sim_steps), else the first measurement of the step path (the loop is closed
    over the step's own nominal prediction).  Returns the mission log the loop implies (and the last measurement)."""
    B, L = wp.shape[:2]
    log = log or dict(leg=np.zeros(B, np.int32) if leg is None else leg.copy(), installed=np.zeros(B, np.int32),
                      leg_code=np.full((B, L), REPLAN_SKIPPED, np.int32), leg_period=np.full((B, L), -1, np.int32))
    leg = log["leg"]
    ar = np.arange(B)
    for k in range(k0, k0 + K):
        if x_meas is None:
            e.sim_steps(1, 2, 5e-3)
            start = None
        else:
            start = x_meas[:, 0:3].copy()
            _, x_meas = e.step(x_meas)
        mask = (e.get_finished() != 0) & (leg < L)
        if mask.any():
            codes = plan(e, wp[ar, np.minimum(leg, L - 1)], mask, start, order, nonlinear, opts)
            sel = np.flatnonzero(mask)
            log["leg_code"][sel, leg[sel]] = codes[sel]
            log["leg_period"][sel, leg[sel]] = k
            log["installed"][sel] += codes[sel] == REPLAN_DONE
            leg[sel] += 1
    return log, x_meas


def mission_run(e, K, x_meas=None, block=None):
    """K periods with the mission active: blocks of sim_steps (the host is not in the loop), or one step call per period."""
    if x_meas is None:
        k = 0
        while k < K:
            n = min(block or K, K - k)
            e.sim_steps(n, 2, 5e-3)
            k += n
        return None
    for _ in range(K):
        _, x_meas = e.step(x_meas)
    return x_meas


LOG_KEYS = ("leg", "installed", "leg_code", "leg_period")


# ------------------------------------------------------------------ cases (engine library, batch)
def case_bit_identity(lib, B, K, L, n_wp=3, size=1.5, precision=0, nonlinear=False, step_path=False, min_installs=1, seed=11, order=4, block=None,
                      **cfg):
    """1. + 2.: after K periods the mission run and the host loop agree bit for bit on state, solver state, plant state, slots and the
    mission log; the window is not vacuous (every quadrotor installed min_installs flights, some period had several finishing)."""
    x0, traj, lens, wp = workload(B, L, n_wp, size, seed)
    opts = dict(max_evaluations=150) if nonlinear else None
    a = start_engine(lib, B, x0, traj, lens, precision=precision, **cfg)
    log, xa = host_loop(a, wp, K, order, nonlinear, opts, x_meas=x0.copy() if step_path else None)
    per_period = np.bincount(log["leg_period"][log["leg_period"] >= 0], minlength=K)
    print(f"host loop: installs per quadrotor min {log['installed'].min()} max {log['installed'].max()}, most finishing in one period {per_period.max()}, "
          f"periods with more than one {int((per_period > 1).sum())}")
    assert log["installed"].min() >= min_installs, log["installed"].min()
    assert per_period.max() > 1
    b = start_engine(lib, B, x0, traj, lens, precision=precision, **cfg)
    b.mission_set(wp, V_MAX, A_MAX, order=order, dt=DT, nonlinear=nonlinear, opts=opts)
    xb = mission_run(b, K, x_meas=x0.copy() if step_path else None, block=block)
    got = b.mission_get()
    assert_same(log, got, LOG_KEYS)
    consumed = got["leg_period"] >= 0
    assert np.array_equal(got["last_code"], np.where(got["leg"] > 0, got["leg_code"][np.arange(B), np.maximum(got["leg"] - 1, 0)], REPLAN_SKIPPED))
    assert np.array_equal(consumed.sum(axis=1), got["leg"])
    assert_same(snapshot(a), snapshot(b))
    if step_path:
        assert np.array_equal(xa, xb)
    if nonlinear:
        flown = got["installed"] > 0
        assert np.isfinite(got["info"][flown]).all() and np.isnan(got["info"][~flown]).all()
    a.close(); b.close()
    return got


def case_no_hold(lib, B, K, L, n_wp=1, size=0.6, seed=12):
    """3. + recording on / off: with the solver field recorded every period, every installed flight contributes exactly one row with
    finished == 1 and the row behind it has cursor 0; the recording changes no result."""
    x0, traj, lens, wp = workload(B, L, n_wp, size, seed)
    runs = []
    for record in (True, False):
        e = start_engine(lib, B, x0, traj, lens)
        e.mission_set(wp, V_MAX, A_MAX)
        if record:
            e.record_start(fields=("solver",), every=1, capacity=K)
        mission_run(e, K, block=7)
        got = e.mission_get()
        if record:
            rec = e.record_get()
            assert rec["period"].tolist() == list(range(K)) and rec["dropped"] == 0
            fin, idx = rec["finished"], rec["idx"]
            assert (got["leg"] < L).all(), "queue exhausted: a longer queue is needed for this check"
            assert (got["leg_code"][got["leg_period"] >= 0] == REPLAN_DONE).all()
            assert np.array_equal(fin.sum(axis=1), got["installed"])          # one finished row per installed flight: nobody held one
            for b in range(B):
                periods = got["leg_period"][b, :got["leg"][b]]
                assert np.array_equal(np.flatnonzero(fin[b]), periods), b
                nxt = periods[periods + 1 < K] + 1
                assert (idx[b, nxt] == 0).all(), b
            assert got["installed"].min() >= 1
            e.record_stop()
        runs.append((snapshot(e), got))
        e.close()
    assert_same(runs[0][0], runs[1][0])
    assert_same(runs[0][1], runs[1][1])


def case_failure_codes(lib, B, K=40, Tmax=300, seed=13):
    """4.: a leg that fails is consumed -- its code is logged, trajectory, cursor and flag stay as they were in that period -- and the
    following leg installs in the next period."""
    L = 3
    x0, traj, lens, wp = workload(B, L, 1, 0.25, seed, Tmax=Tmax)
    wp[0, 0, 0, 1] = np.nan                          # quadrotor 0: leg 0 is not finite
    wp[1, 1, 0] = x0[1, 0:3] + [60.0, -60.0, 30.0]   # quadrotor 1: leg 1 needs more than Tmax rows
    e = start_engine(lib, B, x0, traj, lens)
    plain = start_engine(lib, B, x0, traj, lens)     # never sets a mission
    e.mission_set(wp, V_MAX, A_MAX)
    e.sim_steps(1, 2, 5e-3); plain.sim_steps(1, 2, 5e-3)
    got, t1, l1 = e.mission_get(), *e.get_trajectories()
    tp, lp = plain.get_trajectories()
    assert got["leg_code"][0, 0] == REPLAN_BAD_INPUT and got["leg"][0] == 1 and got["installed"][0] == 0 and got["leg_period"][0, 0] == 0
    assert np.array_equal(t1[0], tp[0]) and l1[0] == lp[0]
    assert e.get_state()["idx"][0] == plain.get_state()["idx"][0] and e.get_finished()[0] == 1 == plain.get_finished()[0]
    assert (got["leg_code"][1:, 0] == REPLAN_DONE).all() and (e.get_finished()[1:] == 0).all()
    e.sim_steps(1, 2, 5e-3)
    got = e.mission_get()
    assert got["leg_code"][0, 1] == REPLAN_DONE and got["leg_period"][0, 1] == 1 and got["installed"][0] == 1
    assert e.get_finished()[0] == 0 and e.get_state()["idx"][0] == 0
    prev = None
    for k in range(2, K):                            # until quadrotor 1 finishes its first flight
        before = (e.get_trajectories(), e.get_state()["idx"].copy())
        e.sim_steps(1, 2, 5e-3)
        got = e.mission_get()
        if got["leg"][1] >= 2:
            prev = before
            break
    assert prev is not None, "quadrotor 1 did not finish its first flight in the window"
    assert got["leg_code"][1, 1] == REPLAN_TOO_LONG and got["leg_period"][1, 1] == k and got["last_code"][1] == REPLAN_TOO_LONG
    (t0, l0), idx0 = prev
    t1, l1 = e.get_trajectories()
    assert np.array_equal(t1[1], t0[1]) and l1[1] == l0[1] and e.get_finished()[1] == 1
    assert e.get_state()["idx"][1] == idx0[1] + 1     # (the step's own advance; the mission launch did not rewind it)
    e.sim_steps(1, 2, 5e-3)
    got = e.mission_get()
    assert got["leg_code"][1, 2] == REPLAN_DONE and got["leg_period"][1, 2] == k + 1 and got["leg"][1] == 3
    assert e.get_finished()[1] == 0 and e.get_state()["idx"][1] == 0
    e.close(); plain.close()
    # ... and the whole run is the host loop's
    a = start_engine(lib, B, x0, traj, lens)
    log, _ = host_loop(a, wp, k + 2)
    b = start_engine(lib, B, x0, traj, lens)
    b.mission_set(wp, V_MAX, A_MAX)
    mission_run(b, k + 2)
    assert_same(log, b.mission_get(), LOG_KEYS)
    assert_same(snapshot(a), snapshot(b))
    a.close(); b.close()


def case_stop_is_parent_behaviour(lib, B, K=12, seed=14):
    """5. (last item): after mission_stop, or on an engine that never set one, a K-period run is what it is without missions."""
    x0, traj, lens, wp = workload(B, 2, 1, 0.5, seed)
    lens[:] = 200
    runs = []
    for mode in ("never", "stopped"):
        e = start_engine(lib, B, x0, traj, lens)
        if mode == "stopped":
            e.mission_set(wp, V_MAX, A_MAX)
            e.mission_stop()
            expect_rc(MPCQ_ERR_STATE, e.mission_stop)
        e.sim_steps(K, 2, 5e-3)
        runs.append(snapshot(e))
        e.close()
    assert_same(runs[0], runs[1])


def case_state_rules(lib, B, K=60, seed=15):
    """6.: argument and state checks; sim_run is refused while a mission is active; an exhausted queue leaves the quadrotor holding."""
    x0, traj, lens, wp = workload(B, 1, 1, 0.25, seed)
    e = Engine(config(B), lib_path=lib)
    expect_rc(MPCQ_ERR_STATE, e.mission_set, wp, V_MAX, A_MAX)                # before set_trajectories
    assert e.lib.mpcq_mission_get(e.h, None, None, None, None, None, None) == MPCQ_ERR_STATE
    e.set_trajectories(traj, lens)
    e.sim_reset(x0)
    for kw in (dict(v_max=0.0), dict(a_max=-1.0), dict(dt=0.0), dict(v_max=float("nan")), dict(a_max=float("inf")), dict(order=1), dict(order=5),
               dict(leg0=np.full(B, 2)), dict(leg0=np.full(B, -1)), dict(nonlinear=True, opts=dict(time_penalty=-1.0))):
        args = dict(wp=wp, v_max=V_MAX, a_max=A_MAX)
        args.update(kw)
        expect_rc(MPCQ_ERR_INVALID, e.mission_set, **args)
    for n_wp in (0, 8):
        expect_rc(MPCQ_ERR_INVALID, e.mission_set, np.zeros((B, 1, n_wp, 3)), V_MAX, A_MAX)
    expect_rc(MPCQ_ERR_INVALID, e.mission_set, np.zeros((B, 0, 1, 3)), V_MAX, A_MAX)
    assert e.lib.mpcq_mission_set(e.h, None, 1, 1, V_MAX, A_MAX, 4, DT, 0, None, None) == MPCQ_ERR_INVALID
    e.sim_run(2, 2, 5e-3)                                                       # no mission: legal
    e.set_trajectories(traj, lens)
    e.sim_reset(x0)
    e.mission_set(wp, V_MAX, A_MAX)
    expect_rc(MPCQ_ERR_STATE, e.sim_run, 2, 2, 5e-3)
    mission_run(e, K)
    got = e.mission_get()
    assert (got["leg"] == 1).all() and (got["installed"] == 1).all() and (got["leg_period"][:, 0] == 0).all()
    assert (e.get_finished() == 1).all(), "the one flight of the queue did not end in the window"
    t0, l0 = e.get_trajectories()
    mission_run(e, 3)                                                           # queue exhausted: holding, nothing is planned
    t1, l1 = e.get_trajectories()
    assert np.array_equal(t0, t1) and np.array_equal(l0, l1) and (e.get_finished() == 1).all()
    assert_same(got, e.mission_get())
    # host replans stay legal while a mission is active and consume no legs
    codes = e.replan(wp[:, 0], V_MAX, A_MAX)
    assert (codes == REPLAN_DONE).all() and (e.mission_get()["leg"] == 1).all()
    e.mission_stop()
    e.sim_run(2, 2, 5e-3)
    e.close()


def case_checkpoint(lib, B, K0, K, L=6, seed=16):
    """7.: state + leg read at period K0 restore a fresh engine (mission_set(leg0 = leg)) that continues bit for bit."""
    x0, traj, lens, wp = workload(B, L, 1, 0.6, seed)
    e = start_engine(lib, B, x0, traj, lens)
    e.mission_set(wp, V_MAX, A_MAX)
    mission_run(e, K0)
    leg = e.mission_get()["leg"]
    assert (leg >= 1).all() and (leg < L).all()
    st, sv, (x, _) = e.get_state(), e.get_solver_state(), e.sim_get_state()
    t, ln = e.get_trajectories()
    f = Engine(config(B), lib_path=lib)
    f.set_trajectories(t, ln)
    f.set_state(**st)
    f.set_solver_state(**sv)
    f.sim_reset(x)
    f.mission_set(wp, V_MAX, A_MAX, leg0=leg)
    mission_run(e, K); mission_run(f, K)
    assert_same(snapshot(e), snapshot(f))
    ge, gf = e.mission_get(), f.mission_get()
    assert np.array_equal(ge["leg"], gf["leg"]) and (ge["leg"] > leg).any()
    new = gf["leg_period"] >= 0                       # the restored engine's log holds the legs consumed since, periods counted from its mission_set
    assert np.array_equal(ge["leg_code"][new], gf["leg_code"][new]) and np.array_equal(ge["leg_period"][new], gf["leg_period"][new] + K0)
    e.close(); f.close()


# ------------------------------------------------------------------ CPU, no library
def test_mission_waypoints_stack_flight_waypoints():
    wp = mission_waypoints(5, 17, 4, 3)
    assert wp.shape == (4, 3, 3, 3)
    for i in range(4):
        for leg in range(3):
            assert np.array_equal(wp[i, leg], flight_waypoints(5, 17 + i, leg))
    assert mission_waypoints(2, 0, 2, 2, num_waypoints=5).shape == (2, 2, 5, 3)


# ------------------------------------------------------------------ lane emulator (CPU)
def test_emu_bit_identity_with_host_loop(emu):
    got = case_bit_identity(emu, 3, 70, L=4, n_wp=1, size=0.5, block=9)
    assert got["installed"].max() >= 2


def test_emu_bit_identity_step_path(emu):
    case_bit_identity(emu, 3, 12, L=2, n_wp=2, size=0.5, step_path=True)


def test_emu_bit_identity_nonlinear(emu):
    case_bit_identity(emu, 3, 6, L=2, n_wp=2, size=0.5, nonlinear=True, order=3)


def test_emu_no_hold_and_recording_invariance(emu):
    case_no_hold(emu, 3, 70, L=6)


def test_emu_failure_codes_consume_a_leg(emu):
    case_failure_codes(emu, 4, K=60)


def test_emu_stop_is_parent_behaviour(emu):
    case_stop_is_parent_behaviour(emu, 3)


def test_emu_state_rules(emu):
    case_state_rules(emu, 3)


def test_emu_checkpoint(emu):
    case_checkpoint(emu, 3, K0=30, K=40)


# ------------------------------------------------------------------ MI355X
gpu = pytest.mark.gpu


@gpu
@pytest.mark.parametrize("precision", [0, 1])
def test_gpu_bit_identity_with_host_loop_b1024(precision):
    case_bit_identity(None, 1024, 500, L=8, precision=precision, min_installs=2, block=50)


@gpu
def test_gpu_bit_identity_nonlinear_b256():
    case_bit_identity(None, 256, 500, L=8, nonlinear=True, order=3, min_installs=2, block=50)


@gpu
def test_gpu_bit_identity_step_path():
    case_bit_identity(None, 256, 400, L=8, n_wp=2, size=1.0, step_path=True, min_installs=2)


@gpu
def test_gpu_no_hold_and_recording_invariance():
    case_no_hold(None, 1024, 200, L=12)


@gpu
def test_gpu_failure_codes_consume_a_leg():
    case_failure_codes(None, 256, K=80)


@gpu
def test_gpu_stop_is_parent_behaviour():
    case_stop_is_parent_behaviour(None, 1024, K=40)


@gpu
def test_gpu_state_rules():
    case_state_rules(None, 256, K=80)


@gpu
def test_gpu_checkpoint():
    case_checkpoint(None, 256, K0=60, K=80, L=10)


def mission_snapshot(B, K, tune=None, seed=17, block=25):
    x0, traj, lens, wp = workload(B, 8, 2, 1.0, seed)
    e = start_engine(None, B, x0, traj, lens, tune=tune)
    e.mission_set(wp, V_MAX, A_MAX)
    mission_run(e, K, block=block)
    out = dict(snapshot(e), **{k: v for k, v in e.mission_get().items()})
    e.close()
    assert out["installed"].min() >= 1
    return out


@gpu
def test_gpu_mission_bit_identical_over_groups():
    assert_same(mission_snapshot(1024, 120, dict(groups=1)), mission_snapshot(1024, 120, dict(groups=4)))


@gpu
def test_gpu_mission_bit_identical_split_plant(monkeypatch):
    monkeypatch.setenv("MPCQ_TUNING", "1")
    monkeypatch.setenv("MPCQ_SPLIT_PLANT", "0")
    a = mission_snapshot(1024, 120)
    monkeypatch.setenv("MPCQ_SPLIT_PLANT", "1")
    assert_same(a, mission_snapshot(1024, 120))

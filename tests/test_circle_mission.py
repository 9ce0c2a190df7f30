"""Circle flights on the device and missions with a kind and limits per leg: mpcq_replan_circle, mpcq_mission_set_legs.  The same cases run
on the lane emulator (CPU, small batches) and on the MI355X (-m gpu, the product library).

Yardsticks:
 * the generator: trajectories.circle_trajectory, the host form that tests/test_sharding.py pins against the reference's
   TrajectoryGenerator (tests/golden/circle_vectors.npz).  Row counts and the constant columns are exact; a position or velocity entry
   may differ by one quantum of the 6-decimal rounding (|d| <= 1e-6 + 1e-12), and at most 1 entry in 1 000 may differ at all: the running
   sums are accumulated in the host's order, so only the device's sin / cos can differ -- a few ulp on values <= ~25, which flips a
   rounding only within ~1e-14 of a half quantum.
 * the mission: the host loop that exists without it, per period: sim_steps(1) (or step(x)); due = finished & (leg < L);
   replan_circle(mask = circle legs due); replan(v, a, mask = ...) once per distinct (v, a) among the waypoint legs due; leg += 1.  A
   mission is the same device functions on the same inputs in the same order, so every comparison against it is bit for bit."""
import os
import subprocess

import numpy as np
import pytest

from mpc_quad_ros_amd import _lib
from mpc_quad_ros_amd.engine import (LEG_CIRCLE, LEG_DTYPE, LEG_WAYPOINTS, REPLAN_BAD_INPUT, REPLAN_DONE, REPLAN_SKIPPED, REPLAN_TOO_LONG,
                                     Engine)
from mpc_quad_ros_amd.params import EngineConfig, hummingbird, rgp_basis_linspace
from mpc_quad_ros_amd.trajectories import circle_trajectory, mission_legs

HERE = os.path.dirname(os.path.abspath(__file__))
EMU_DIR = os.path.join(HERE, "wave_emu")
EMU = os.path.join(EMU_DIR, "libmpcq_emu.so")
GOLDEN = os.path.join(HERE, "golden", "circle_vectors.npz")
HOVER = np.array([0, 0, 3.0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0])
MPCQ_ERR_INVALID, MPCQ_ERR_STATE = -1, -3
DT = 0.01
QUANTUM = 1e-6 + 1e-12
PV = [0, 1, 2, 7, 8]            # the columns a circle computes: position, x / y velocity
CONST = [3, 4, 5, 6, 9, 10, 11, 12]   # q, z velocity, body rates
CONST_ROW = np.array([1.0, 0, 0, 0, 0, 0, 0, 0])


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


def hover_slots(B, Tmax, seed, spread=0.3):
    """Start points and hover slots of two rows: everybody finishes in the first period."""
    rng = np.random.default_rng(seed)
    x0 = np.tile(HOVER, (B, 1))
    x0[:, 0:3] += rng.uniform(-spread, spread, (B, 3))
    return x0, np.repeat(x0[:, None, :], Tmax, axis=1).copy(), np.full(B, 2, np.int32)


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


LOG_KEYS = ("leg", "installed", "leg_code", "leg_period")


# ------------------------------------------------------------------ 1. the generator against the pinned host generator
# radius x v_max of the issue, all twelve, and four repeats at other start points; index 4 (radius 10 at 8 m/s: 1 571 rows of 0.01 s as
# an acc_dec circle) is the one flight that does not fit GEN_TMAX.  The last three carry the parameter sets of circle_vectors.npz.
GEN_COMBOS = [(r, v) for r in (5.0, 10.0, 2.5) for v in (8.0, 10.0, 12.0, 15.0)] + [(2.5, 15.0), (10.0, 10.0), (5.0, 8.0), (10.0, 12.0)]
GEN_TMAX = 1400
GEN_TOO_LONG = 4
# kind, dt, t_max, index and key of the golden flight, its start point
GEN_CALLS = [("acc_dec", 0.01, 10.0, 13, "ad_x", (0.0, 0.0, 0.0)),
             ("constant", 0.05, 10.0, 14, "const_x", (1.0, -2.0, 3.0)),
             ("accelerating", 0.1, 30.0, 15, "acc_x", (0.0, 0.0, 3.0)),
             ("accelerating", 0.01, 10.0, None, None, None)]


def compare_flight(got, n, want, what):
    """Rows [0, n) of slot `got` against the flight `want`; returns (entries that differ, entries compared)."""
    assert n == len(want), (what, n, len(want))
    assert np.array_equal(got[:n, CONST], np.tile(CONST_ROW, (n, 1))), what
    assert np.array_equal(got[n:], np.tile(got[n - 1], (len(got) - n, 1))), what
    d = np.abs(got[:n, PV] - want[:, PV])
    print(f"{what}: rows {n}, entries that differ {int((d != 0).sum())} of {d.size}, largest difference {d.max():.3e}")
    assert d.max() <= QUANTUM, (what, d.max())
    return int((d != 0).sum()), d.size


def case_generator(lib):
    B = len(GEN_COMBOS)
    golden = np.load(GOLDEN)
    radius, v_max = np.array([c[0] for c in GEN_COMBOS]), np.array([c[1] for c in GEN_COMBOS])
    x0, traj, lens = hover_slots(B, GEN_TMAX, 21)
    e = Engine(config(B, nb=0), lib_path=lib)
    e.set_trajectories(traj, lens)
    for kind, dt, t_max, gi, gkey, gstart in GEN_CALLS:
        start = np.random.default_rng(22).uniform(-20.0, 20.0, (B, 3))
        if gi is not None:
            start[gi] = gstart
        codes = e.replan_circle(radius, v_max, kind, dt, t_max, start=start, mask=np.ones(B, np.int32))
        t, ln = e.get_trajectories()
        differ = total = 0
        for b in range(B):
            want, _ = circle_trajectory(kind, radius[b], v_max[b], dt, t_max, start[b])
            if kind == "acc_dec" and b == GEN_TOO_LONG:
                assert len(want) > GEN_TMAX and codes[b] == REPLAN_TOO_LONG
                continue
            assert codes[b] == REPLAN_DONE, (kind, b, codes[b])
            n, m = compare_flight(t[b], ln[b], want, f"{kind} dt {dt} radius {radius[b]} v_max {v_max[b]}")
            differ += n; total += m
            if b == gi:   # ... and against the reference's own output
                n, m = compare_flight(t[b], ln[b], golden[gkey], f"{kind} against {gkey} of circle_vectors.npz")
                assert 1000 * n <= m, (gkey, n, m)
        print(f"{kind} dt {dt}: {differ} of {total} entries differ from circle_trajectory")
        assert 1000 * differ <= total, (kind, differ, total)
        st = e.get_state()
        done = codes == REPLAN_DONE
        assert (st["idx"][done] == 0).all() and (e.get_finished()[done] == 0).all()
    e.close()


# ------------------------------------------------------------------ 2. codes and state
def case_codes_and_state(lib, B=8, Tmax=400):
    x0, traj, lens = hover_slots(B, Tmax, 23)
    e = Engine(config(B), lib_path=lib)
    one = np.ones(B)
    expect_rc(MPCQ_ERR_STATE, e.replan_circle, one, one, start=x0[:, 0:3], mask=one)          # before set_trajectories
    e.set_trajectories(traj, lens)
    expect_rc(MPCQ_ERR_STATE, e.replan_circle, one, one, mask=one)                            # plant position before sim_reset
    e.sim_reset(x0)
    for kw in (dict(dt=0.0), dict(dt=-0.01), dict(dt=float("nan")), dict(dt=float("inf")), dict(kind="accelerating", t_max=0.0),
               dict(kind="accelerating", t_max=float("inf"))):
        expect_rc(MPCQ_ERR_INVALID, e.replan_circle, one, one, mask=one, **kw)
    out = np.zeros(B, np.int32)
    for kind in (-1, 3):
        assert e.lib.mpcq_replan_circle(e.h, None, _lib.d(one), _lib.d(one), kind, DT, 10.0, None, _lib.i(out)) == MPCQ_ERR_INVALID
    assert e.lib.mpcq_replan_circle(e.h, None, None, _lib.d(one), 0, DT, 10.0, None, _lib.i(out)) == MPCQ_ERR_INVALID
    assert e.lib.mpcq_replan_circle(e.h, None, _lib.d(one), None, 0, DT, 10.0, None, _lib.i(out)) == MPCQ_ERR_INVALID
    with pytest.raises(ValueError):
        e.replan_circle(one, one, kind="spiral")
    e.sim_steps(3, 2, 5e-3)   # iterate, RGP and tracking accumulators hold something; everybody has finished the hover slot
    assert (e.get_finished() == 1).all()
    before = snapshot(e)
    # 0: NaN start, 1: radius 0, 2: negative v_max, 3: does not fit (radius 10 at 8 m/s), 4: not selected, 5..: fly
    start = x0[:, 0:3] + 0.5
    start[0, 1] = np.nan
    radius, v_max = np.full(B, 0.5), np.full(B, 8.0)
    radius[1], v_max[2], radius[3] = 0.0, -8.0, 10.0
    mask = np.ones(B, np.int32)
    mask[4] = 0
    codes = e.replan_circle(radius, v_max, start=start, mask=mask)
    assert codes[:5].tolist() == [REPLAN_BAD_INPUT, REPLAN_BAD_INPUT, REPLAN_BAD_INPUT, REPLAN_TOO_LONG, REPLAN_SKIPPED]
    assert (codes[5:] == REPLAN_DONE).all()
    after = snapshot(e)
    untouched = [k for k in before if k not in ("traj", "len", "st_idx", "sv_finished")]
    assert_same(before, after, untouched)                     # iterate, RGP, x_pred_prev, QP status, tracking accumulators, plant
    for k in ("traj", "len", "st_idx", "sv_finished"):
        assert np.array_equal(before[k][:5], after[k][:5]), k   # a negative code (and SKIPPED) leaves the slot, the cursor and the flag
    for b in range(5, B):
        want, _ = circle_trajectory("acc_dec", radius[b], v_max[b], DT, start_point=start[b])
        compare_flight(after["traj"][b], after["len"][b], want, f"quadrotor {b}")
    assert (after["st_idx"][5:] == 0).all() and (after["sv_finished"][5:] == 0).all()
    # mask None: the finished flags select (0..4 still finished); start None: the plant position
    codes = e.replan_circle(0.5, 8.0)
    assert (codes[:5] == REPLAN_DONE).all() and (codes[5:] == REPLAN_SKIPPED).all()
    t, ln = e.get_trajectories()
    for b in range(5):
        want, _ = circle_trajectory("acc_dec", 0.5, 8.0, DT, start_point=after["x"][b, 0:3])
        compare_flight(t[b], ln[b], want, f"quadrotor {b} from the plant position")
    assert (e.get_finished() == 0).all()
    e.close()


def case_legs_argument_rules(lib, B=3, L=2):
    x0, traj, lens = hover_slots(B, 100, 24)
    wp = x0[:, None, None, 0:3] + np.zeros((B, L, 1, 3))
    good = mission_legs(B, L, 8.0, kind=[["circle", "waypoints"]], radius=0.5)
    e = Engine(config(B), lib_path=lib)
    expect_rc(MPCQ_ERR_STATE, e.mission_set_legs, good, wp)                                    # before set_trajectories
    e.set_trajectories(traj, lens)
    e.sim_reset(x0)

    def bad(field, where, value):
        t = good.copy()
        t[field][where] = value
        return t
    for legs in (bad("kind", (1, 0), 2), bad("kind", (2, 1), -1), bad("reserved", (0, 1), 1), bad("v_max", (1, 1), 0.0),
                 bad("v_max", (0, 0), float("nan")), bad("a_max", (2, 0), float("inf")), bad("a_max", (2, 1), -1.0),
                 bad("radius", (1, 0), 0.0), bad("radius", (0, 0), float("nan"))):
        expect_rc(MPCQ_ERR_INVALID, e.mission_set_legs, legs, wp)
    expect_rc(MPCQ_ERR_INVALID, e.mission_set_legs, good, None)                                # a waypoint leg without waypoints
    for kw in (dict(dt=0.0), dict(order=5), dict(leg0=np.full(B, L + 1)), dict(nonlinear=True, opts=dict(time_penalty=-1.0))):
        expect_rc(MPCQ_ERR_INVALID, e.mission_set_legs, good, wp, **kw)
    expect_rc(MPCQ_ERR_INVALID, e.mission_set_legs, good, np.zeros((B, L, 8, 3)))
    assert e.lib.mpcq_mission_set_legs(e.h, None, _lib.d(wp), L, 1, 4, DT, 0, None, None) == MPCQ_ERR_INVALID
    with pytest.raises(ValueError):
        e.mission_set_legs(dict(kind=LEG_CIRCLE, v_max=np.full((B, L), 8.0)))                  # no a_max
    expect_rc(MPCQ_ERR_STATE, e.mission_stop)                                                  # none of the refused calls set a mission
    e.mission_set_legs(good, wp)                                                               # (the radius of a waypoint leg is not read: 0)
    e.mission_set_legs(dict(kind="circle", v_max=np.full((B, L), 8.0), a_max=8.0, radius=0.5))  # circles only: no waypoints
    assert e.mission_get()["leg_code"].shape == (B, L)
    e.mission_stop()
    e.close()


# ------------------------------------------------------------------ 3. mission equals host loop
def mixed_queue(B, L, n_wp, seed, radii, speeds, size, Tmax):
    """Kinds and limits that vary per quadrotor and leg: roughly every other leg a circle; one circle that does not fit Tmax
    (quadrotor 0, leg 1) and one waypoint leg that is not finite (quadrotor 1, leg 0)."""
    rng = np.random.default_rng(seed)
    x0, traj, lens = hover_slots(B, Tmax, seed + 100)
    kind = rng.integers(0, 2, (B, L)).astype(np.int32)
    kind[0, 1], kind[1, 0] = LEG_CIRCLE, LEG_WAYPOINTS
    kind[2 % B, :] = [LEG_CIRCLE, LEG_WAYPOINTS, LEG_CIRCLE][:L]
    v = rng.choice(speeds, (B, L))
    legs = mission_legs(B, L, v, a_max=rng.choice(speeds, (B, L)), kind=kind, radius=rng.choice(radii, (B, L)))
    legs["radius"][0, 1] = 40.0          # 4 pi 40 / v / dt rows: more than Tmax at every speed used here
    wp = x0[:, None, None, 0:3] + rng.uniform(-size, size, (B, L, n_wp, 3))
    wp[1, 0, 0, 2] = np.nan
    return x0, traj, lens, legs, wp


def host_loop(e, legs, wp, K, order=4, nonlinear=False, opts=None, x_meas=None):
    B, L = legs.shape
    log = dict(leg=np.zeros(B, np.int32), installed=np.zeros(B, np.int32), leg_code=np.full((B, L), REPLAN_SKIPPED, np.int32),
               leg_period=np.full((B, L), -1, np.int32))
    leg, ar = log["leg"], np.arange(B)
    for k in range(K):
        if x_meas is None:
            e.sim_steps(1, 2, 5e-3)
            start = None
        else:
            start = x_meas[:, 0:3].copy()
            _, x_meas = e.step(x_meas)
        due = (e.get_finished() != 0) & (leg < L)
        if not due.any():
            continue
        now = legs[ar, np.minimum(leg, L - 1)]
        wp_now = wp[ar, np.minimum(leg, L - 1)]
        codes = np.full(B, REPLAN_SKIPPED, np.int32)
        circ = due & (now["kind"] == LEG_CIRCLE)
        if circ.any():
            c = e.replan_circle(np.where(circ, now["radius"], 1.0), now["v_max"], "acc_dec", DT, start=start, mask=circ)
            codes[circ] = c[circ]
        way = due & (now["kind"] == LEG_WAYPOINTS)
        for v, a in sorted(set(zip(now["v_max"][way].tolist(), now["a_max"][way].tolist()))):
            m = way & (now["v_max"] == v) & (now["a_max"] == a)
            if nonlinear:
                c = e.replan_nonlinear(wp_now, v, a, DT, order, start=start, mask=m, opts=opts)[0]
            else:
                c = e.replan(wp_now, v, a, DT, order, start=start, mask=m)
            codes[m] = c[m]
        sel = np.flatnonzero(due)
        log["leg_code"][sel, leg[sel]] = codes[sel]
        log["leg_period"][sel, leg[sel]] = k
        log["installed"][sel] += codes[sel] == REPLAN_DONE
        leg[sel] += 1
    return log, x_meas


def mission_run(e, K, x_meas=None, block=None):
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


def case_mission_equals_host_loop(lib, B, K, radii, speeds, size, Tmax, n_wp=1, nonlinear=False, step_path=False, order=4, seed=31, block=None,
                                  min_consumed=2, **cfg):
    L = 3
    x0, traj, lens, legs, wp = mixed_queue(B, L, n_wp, seed, radii, speeds, size, Tmax)
    opts = dict(max_evaluations=150) if nonlinear else None
    a = start_engine(lib, B, x0, traj, lens, **cfg)
    log, xa = host_loop(a, legs, wp, K, order, nonlinear, opts, x_meas=x0.copy() if step_path else None)
    print(f"host loop: legs consumed per quadrotor min {log['leg'].min()} max {log['leg'].max()}, installs {log['installed'].tolist()[:8]}")
    assert log["leg"].min() >= min_consumed, log["leg"]
    assert log["leg_code"][1, 0] == REPLAN_BAD_INPUT and log["leg_period"][1, 0] == 0
    if log["leg"][0] >= 2:
        assert log["leg_code"][0, 1] == REPLAN_TOO_LONG
    consumed = log["leg_period"] >= 0
    assert (log["leg_code"][consumed & (legs["kind"] == LEG_CIRCLE)] == REPLAN_DONE).sum() >= 1
    assert (log["leg_code"][consumed & (legs["kind"] == LEG_WAYPOINTS)] == REPLAN_DONE).sum() >= 1
    b = start_engine(lib, B, x0, traj, lens, **cfg)
    b.mission_set_legs(legs, wp, order=order, dt=DT, nonlinear=nonlinear, opts=opts)
    xb = mission_run(b, K, x_meas=x0.copy() if step_path else None, block=block)
    got = b.mission_get()
    assert_same(log, got, LOG_KEYS)
    assert_same(snapshot(a), snapshot(b))
    if step_path:
        assert np.array_equal(xa, xb)
    ar = np.arange(B)
    assert np.array_equal(got["last_code"], np.where(got["leg"] > 0, got["leg_code"][ar, np.maximum(got["leg"] - 1, 0)], REPLAN_SKIPPED))
    if nonlinear:   # info: the row of the last installed flight, NaN if that was a circle (or none was installed)
        for q in range(B):
            done = [l for l in range(got["leg"][q]) if got["leg_code"][q, l] == REPLAN_DONE]
            finite = bool(done) and legs["kind"][q, done[-1]] == LEG_WAYPOINTS
            assert np.isfinite(got["info"][q]).all() if finite else np.isnan(got["info"][q]).all(), q
    else:
        assert np.isnan(got["info"]).all()
    a.close(); b.close()
    return got


# ------------------------------------------------------------------ 4. recorder interplay
def case_recorder(lib, B, K, radius, v_max, Tmax):
    """A mission of one circle leg per quadrotor under the recorder: the finishing period shows finished = 1, the next row cursor 0 and
    x_ref = row 0 of the circle that starts where the plant stood behind the finishing period."""
    x0, traj, lens = hover_slots(B, Tmax, 41)
    e = start_engine(lib, B, x0, traj, lens)
    e.mission_set_legs(mission_legs(B, 1, v_max, kind="circle", radius=radius))
    e.record_start(fields=("solver", "x_ref", "x_odom"), every=1, capacity=K)
    mission_run(e, K, block=5)
    rec, got = e.record_get(), e.mission_get()
    assert rec["period"].tolist() == list(range(K)) and rec["dropped"] == 0
    assert (got["leg_code"][:, 0] == REPLAN_DONE).all() and (got["installed"] == 1).all()
    t, ln = e.get_trajectories()
    for b in range(B):
        p = got["leg_period"][b, 0]
        assert p + 1 < K
        assert rec["finished"][b, p] == 1 and rec["finished"][b, p + 1] == 0
        assert rec["idx"][b, p + 1] == 0
        assert np.array_equal(rec["x_ref"][b, p + 1], t[b, 0])
        want, _ = circle_trajectory("acc_dec", radius, v_max, DT, start_point=rec["x_odom"][b, p + 1, 0:3])
        compare_flight(t[b], ln[b], want, f"quadrotor {b}")
        assert np.abs(rec["x_ref"][b, p + 1] - want[0]).max() <= QUANTUM
    e.record_stop()
    e.close()


# ------------------------------------------------------------------ 5. the old entry point
def case_old_entry_point(lib, B, K, L=3, n_wp=2, size=0.5, nonlinear=False, order=4, seed=51):
    rng = np.random.default_rng(seed)
    x0, traj, lens = hover_slots(B, 400, seed)
    wp = x0[:, None, None, 0:3] + rng.uniform(-size, size, (B, L, n_wp, 3))
    opts = dict(max_evaluations=150) if nonlinear else None
    runs = []
    for new in (False, True):
        e = start_engine(lib, B, x0, traj, lens)
        if new:
            e.mission_set_legs(mission_legs(B, L, 12.0, a_max=9.0), wp, order=order, dt=DT, nonlinear=nonlinear, opts=opts)
        else:
            e.mission_set(wp, 12.0, 9.0, order=order, dt=DT, nonlinear=nonlinear, opts=opts)
        mission_run(e, K, block=7)
        runs.append(dict(snapshot(e), **e.mission_get()))
        e.close()
    assert runs[0]["installed"].min() >= 1
    assert_same(runs[0], runs[1])


# ------------------------------------------------------------------ 6. closed loop on the node's circle
def case_closed_loop_circle(lib, B=1, radius=10.0, v_max=10.0, slack=100):
    """An acc_dec circle of radius 10 at 10 m/s from hover under the on-device plant is flown to its end: the finished flag is set within
    len + slack periods of the install and the next leg is consumed.  slack: the flag needs the cursor on the last row (len - 1 periods
    behind the install) and the quadrotor within the finish radius (1 m) of the reference, which ends at rest -- 1 s for the lag at the
    end of the deceleration to decay; no tracking-error bound (the reference logs give none for this plant)."""
    want, _ = circle_trajectory("acc_dec", radius, v_max, DT)
    n = len(want)
    x0, traj, lens = hover_slots(B, n + 8, 61)
    e = start_engine(lib, B, x0, traj, lens)
    e.mission_set_legs(mission_legs(B, 2, v_max, kind="circle", radius=[[radius, 0.5]]))
    mission_run(e, n + slack + 2, block=64)
    got = e.mission_get()
    _, ln = e.get_trajectories()
    print(f"circle of {n} rows: installed in period {got['leg_period'][:, 0].tolist()}, next leg consumed in period {got['leg_period'][:, 1].tolist()}")
    assert (got["leg_period"][:, 0] == 0).all() and (got["leg_code"] == REPLAN_DONE).all() and (got["leg"] == 2).all()
    flown = got["leg_period"][:, 1] - got["leg_period"][:, 0]
    assert (flown >= n - 1).all() and (flown <= n + slack).all(), flown
    e.close()


# ------------------------------------------------------------------ CPU, no library
def test_mission_legs_builds_a_speed_sweep():
    t = mission_legs(4, 3, np.array([[3.0], [6.0], [9.0], [12.0]]))
    assert t.dtype == LEG_DTYPE and t.shape == (4, 3) and t.dtype.itemsize == 32
    assert (t["kind"] == LEG_WAYPOINTS).all() and (t["reserved"] == 0).all() and (t["radius"] == 0).all()
    assert np.array_equal(t["v_max"], np.repeat([[3.0], [6.0], [9.0], [12.0]], 3, axis=1)) and np.array_equal(t["a_max"], t["v_max"])
    t = mission_legs(2, 3, [8.0, 10.0, 12.0], a_max=6.0, kind=["circle", "waypoints", "circle"], radius=10.0)
    assert t["kind"].tolist() == [[LEG_CIRCLE, LEG_WAYPOINTS, LEG_CIRCLE]] * 2 and t["radius"].tolist() == [[10.0, 0.0, 10.0]] * 2
    assert t["v_max"].tolist() == [[8.0, 10.0, 12.0]] * 2 and (t["a_max"] == 6.0).all()


# ------------------------------------------------------------------ lane emulator (CPU)
EMU_RADII, EMU_SPEEDS = (0.15, 0.2, 0.3), (6.0, 8.0, 10.0)   # flights of 19 .. 63 rows: several per quadrotor in a short window


def test_emu_generator_matches_host_generator(emu):
    case_generator(emu)


def test_emu_codes_and_state(emu):
    case_codes_and_state(emu)


def test_emu_legs_argument_rules(emu):
    case_legs_argument_rules(emu)


def test_emu_mission_equals_host_loop(emu):
    case_mission_equals_host_loop(emu, 4, 90, EMU_RADII, EMU_SPEEDS, 0.5, 300, block=9)


def test_emu_mission_equals_host_loop_nonlinear(emu):
    case_mission_equals_host_loop(emu, 3, 45, EMU_RADII, EMU_SPEEDS, 0.5, 300, n_wp=2, nonlinear=True, order=3)


def test_emu_mission_equals_host_loop_step_path(emu):
    case_mission_equals_host_loop(emu, 3, 45, EMU_RADII, EMU_SPEEDS, 0.5, 300, step_path=True)


def test_emu_mission_equals_host_loop_groups(emu):
    case_mission_equals_host_loop(emu, 4, 75, EMU_RADII, EMU_SPEEDS, 0.5, 300, block=9, tune=dict(groups=2))


def test_emu_recorder_interplay(emu):
    case_recorder(emu, 3, 8, 0.3, 8.0, 100)


def test_emu_old_entry_point(emu):
    case_old_entry_point(emu, 3, 40)


def test_emu_old_entry_point_nonlinear(emu):
    case_old_entry_point(emu, 2, 6, L=2, nonlinear=True, order=3)


def test_emu_closed_loop_circle(emu):
    case_closed_loop_circle(emu)


# ------------------------------------------------------------------ MI355X
gpu = pytest.mark.gpu
GPU_RADII, GPU_SPEEDS = (1.0, 2.5), (8.0, 10.0, 12.0)   # flights of 105 .. 393 rows


@gpu
def test_gpu_generator_matches_host_generator():
    case_generator(None)


@gpu
def test_gpu_codes_and_state():
    case_codes_and_state(None, B=64)


@gpu
def test_gpu_legs_argument_rules():
    case_legs_argument_rules(None, B=64)


@gpu
@pytest.mark.parametrize("precision", [0, 1])
def test_gpu_mission_equals_host_loop_b256(precision):
    case_mission_equals_host_loop(None, 256, 900, GPU_RADII, GPU_SPEEDS, 1.5, 600, n_wp=3, block=50, precision=precision)


@gpu
def test_gpu_mission_equals_host_loop_nonlinear():
    case_mission_equals_host_loop(None, 128, 900, GPU_RADII, GPU_SPEEDS, 1.5, 600, n_wp=3, nonlinear=True, order=3, block=50)


@gpu
def test_gpu_mission_equals_host_loop_step_path():
    case_mission_equals_host_loop(None, 128, 700, GPU_RADII, GPU_SPEEDS, 1.0, 600, n_wp=2, step_path=True)


@gpu
def test_gpu_mission_equals_host_loop_groups():
    case_mission_equals_host_loop(None, 1024, 900, GPU_RADII, GPU_SPEEDS, 1.5, 600, n_wp=2, block=50, tune=dict(groups=4))


@gpu
def test_gpu_recorder_interplay():
    case_recorder(None, 256, 12, 2.5, 10.0, 400)


@gpu
def test_gpu_old_entry_point():
    case_old_entry_point(None, 256, 300, L=6, n_wp=3, size=1.5)


@gpu
def test_gpu_old_entry_point_nonlinear():
    case_old_entry_point(None, 128, 300, L=6, n_wp=2, size=1.0, nonlinear=True, order=3)


@gpu
def test_gpu_closed_loop_circle():
    case_closed_loop_circle(None, B=64)

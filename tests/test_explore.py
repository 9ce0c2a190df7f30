"""Exploration on the device (mpcq_explore_start / _get / _stop, Engine.explore_*, params.explore_*): every quadrotor keeps the envelope of
the body-frame velocities it has flown, and in the period a flight ends the limits of its next mission leg come from that envelope by the
reference's rule.  The same cases run on the lane emulator (CPU, B <= 6) and on the MI355X (-m gpu, the product library).

Shapes: N = 10, nb = 10, control period sim_steps(1, 2, 5e-3), L = 3 (L = 1 in the rules case).  On the GPU: B = 70 (two blocks of the
launch, the second ragged), waypoint legs of 3 waypoints within +-1.5 m as test_mission.workload makes them, step 2 m/s.  Such a flight is
550 .. 1 400 periods at these limits and the emulator runs about three periods of five quadrotors a second, so the emulator flies the
emulator shapes of tests/test_mission.py -- one waypoint within +-0.3 m, 50 .. 110 periods a flight, step 3 m/s -- through the same case
functions.

Yardsticks:
 * the rule: the reference's own Explorer methods (tests/golden/explore_vectors.npz, make_explore_golden.py), exactly -- only additions,
   comparisons and abs are involved; the clips and the axis mask against expectations written by hand.
 * the envelope: np.min / np.max over the recorder's v_body rows (MPCQ_RECORD_DRAG), exactly.
 * the policy: the host loop that exists without the feature, per period: sim_steps(1) (or step(x)); due = finished & (leg < L); the
   envelope from the loop's own recording; explore_velocity; replan_circle / replan with mask once per distinct (v, a) among the due
   legs; leg += 1.  Bit for bit: the device runs the same device functions on the same inputs in the same order."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from mpc_quad_ros_amd import _lib
from mpc_quad_ros_amd.engine import LEG_CIRCLE, LEG_WAYPOINTS, REPLAN_DONE, REPLAN_SKIPPED, Engine
from mpc_quad_ros_amd.params import (EXPLORE_CUMULATIVE, EXPLORE_LAST_FLIGHT, EXPLORE_RULE_DTYPE, explore_rules, explore_velocity,
                                     fleet_sample)
from mpc_quad_ros_amd.trajectories import mission_legs
from test_circle_mission import DT, LOG_KEYS, assert_same, config, expect_rc, snapshot, start_engine
from test_fleet import header_struct
from test_mission import workload

HERE = os.path.dirname(os.path.abspath(__file__))
EMU_DIR = os.path.join(HERE, "wave_emu")
EMU = os.path.join(EMU_DIR, "libmpcq_emu.so")
GOLDEN = os.path.join(HERE, "golden", "explore_vectors.npz")
MPCQ_ERR_INVALID, MPCQ_ERR_STATE = -1, -3
L = 3
# what a run flies: (n_wp, size of the legs [m], step [m/s], circle radius [m], Tmax)
EMU_SHAPE = dict(n_wp=1, size=0.3, step=3.0, radius=0.15, Tmax=400)
GPU_SHAPE = dict(n_wp=3, size=1.5, step=2.0, radius=1.0, Tmax=2400)


@pytest.fixture(scope="module")
def emu():
    subprocess.check_call(["make", "-C", EMU_DIR], stdout=subprocess.DEVNULL)
    return EMU


def make_rules(B, step, mode=None):
    """Rules that take every branch, by quadrotor index mod 5: 0 desired far above reach (always explored + step), 1 desired < step
    (always desired), 2 v_limit < step (v_max clipped, a_max not), 3 a_limit < v_limit (a_max clipped only), 4 axes = 3.  mode None: last
    flight and cumulative alternate, but kind 0 is always last flight: it is asked for a new v_max on every leg, and a cumulative
    envelope stays where it is when a flight does not reach further than the one before on the axis that limits it."""
    kind = np.arange(B) % 5
    r = explore_rules(B, step=step, desired=50.0, v_limit=30.0, a_limit=30.0, mode=np.arange(B) % 2 if mode is None else mode)
    if mode is None:
        r["mode"][kind == 0] = EXPLORE_LAST_FLIGHT
    r["desired"][kind == 1] = 0.9 * step
    r["v_limit"][kind == 2] = 0.9 * step
    r["a_limit"][kind == 3] = 0.8 * step
    r["axes"][kind == 4] = 3
    return r


def make_mask(B):
    """Every leg explored but leg 1 of the quadrotors 3 mod 5: that one flies the limits of the table."""
    m = np.ones((B, L), np.uint8)
    m[3::5, 1] = 0
    return m


def make_queue(B, shape, seed, circle=False, legs_n=L):
    x0, traj, lens, wp = workload(B, legs_n, shape["n_wp"], shape["size"], seed, Tmax=shape["Tmax"])
    kind = np.full((B, legs_n), LEG_WAYPOINTS, np.int32)
    if circle:
        kind[:, 1] = LEG_CIRCLE
    legs = mission_legs(B, legs_n, 12.0, a_max=9.0, kind=kind, radius=shape["radius"])
    return x0, traj, lens, wp, legs


def envelope(rec, mode):
    """(env [B, 3, 2], samples [B]) of a recording: min and max of the v_body rows -- all of them (cumulative), or those since the last
    row whose cursor is 0 (last flight)."""
    v, idx = rec["v_body"], rec["idx"]
    B, T = idx.shape
    env, samples = np.zeros((B, 3, 2)), np.zeros(B, np.int64)
    for b in range(B):
        zero = np.flatnonzero(idx[b] == 0)
        t0 = zero[-1] if mode[b] == EXPLORE_LAST_FLIGHT and len(zero) else 0
        if T > t0:
            env[b, :, 0], env[b, :, 1], samples[b] = v[b, t0:].min(axis=0), v[b, t0:].max(axis=0), T - t0
    return env, samples


def run_periods(e, K, x_meas=None, block=50):
    if x_meas is None:
        k = 0
        while k < K:
            n = min(block, K - k)
            e.sim_steps(n, 2, 5e-3)
            k += n
        return None
    for _ in range(K):
        _, x_meas = e.step(x_meas)
    return x_meas


# ------------------------------------------------------------------ 1. the rule against the reference (CPU, no library)
def test_rule_matches_reference_vectors():
    g = np.load(GOLDEN, allow_pickle=False)
    env, n = g["env"], len(g["env"])
    assert n >= 300
    assert (env[0] == 0).all() and (g["explored"][0] == 0)                                    # the all-zero envelope
    vabs = np.maximum(0.0, np.maximum(env[:, :, 1], np.abs(env[:, :, 0])))
    srt = np.sort(vabs, axis=1)
    assert (srt[:, 0] == srt[:, 1]).sum() >= 10                                               # ties between axes
    assert (g["explored"] + g["step"] == g["desired"]).sum() >= 40                            # the strict `<` at equality
    rules = explore_rules(n, step=g["step"], desired=g["desired"], v_limit=np.inf, a_limit=np.inf)
    explored, v, a = explore_velocity(env, np.ones(n, np.int64), rules)
    assert np.array_equal(explored, g["explored"]) and np.array_equal(v, g["velocity"]) and np.array_equal(a, g["velocity"])
    # samples == 0: the envelope reads as all zero, whatever it holds
    explored, v, _ = explore_velocity(env, np.zeros(n, np.int64), rules)
    assert (explored == 0).all() and np.array_equal(v, np.where(g["step"] < g["desired"], g["step"], g["desired"]))


def test_rule_clips_and_axis_mask():
    env = np.array([[[-1.0, 4.0], [-6.0, 2.0], [-0.5, 0.25]]] * 8)                            # reach 4, 6, 0.5
    rules = explore_rules(8, step=2.0, desired=7.0)
    rules["axes"] = [7, 1, 2, 4, 3, 5, 6, 7]
    rules["v_limit"][7], rules["a_limit"][7] = 2.25, 30.0
    rules["v_limit"][0], rules["a_limit"][0] = 30.0, 1.5
    rules["desired"][1], rules["desired"][2] = 6.0, 20.0
    explored, v, a = explore_velocity(env, np.full(8, 3), rules)
    assert explored.tolist() == [0.5, 4.0, 6.0, 0.5, 4.0, 0.5, 0.5, 0.5]
    assert v.tolist() == [2.5, 6.0, 8.0, 2.5, 6.0, 2.5, 2.5, 2.25]                            # 4 + 2 is not < 6: desired; the last one clipped
    assert a.tolist() == [1.5, 6.0, 8.0, 2.5, 6.0, 2.5, 2.5, 2.5]                             # the first one clipped, v is not
    d = explore_rules(3)                                                                      # the reference's numbers
    assert (d["step"] == 10.0).all() and (d["desired"] == 20.0).all() and (d["v_limit"] == 30.0).all() and (d["a_limit"] == 30.0).all()
    assert (d["mode"] == EXPLORE_LAST_FLIGHT).all() and (d["axes"] == 7).all()
    assert explore_velocity(np.zeros((3, 3, 2)), np.zeros(3), d)[1].tolist() == [10.0] * 3    # run 1 of the reference: gpe is None


def test_rule_dtype_matches_header():
    sizes = {"double": (8, np.float64), "int32_t": (4, np.int32)}
    fields = header_struct("mpcq_explore_rule")
    assert [f[0] for f in fields] == list(EXPLORE_RULE_DTYPE.names)
    off = 0
    for name, ctype, count in fields:
        size, dt = sizes[ctype]
        off = -(-off // size) * size
        assert EXPLORE_RULE_DTYPE.fields[name][1] == off and EXPLORE_RULE_DTYPE.fields[name][0] == dt and count == 1, name
        off += size
    assert EXPLORE_RULE_DTYPE.itemsize == -(-off // 8) * 8 == 40


# ------------------------------------------------------------------ 2. the envelope against the recorder
def case_envelope(lib, B, K, shape, mode):
    x0, traj, lens, wp, legs = make_queue(B, shape, 81)
    e = start_engine(lib, B, x0, traj, lens)
    e.mission_set_legs(legs, wp, dt=DT)
    rules = make_rules(B, shape["step"], mode=mode)
    e.explore_start(rules)
    got = e.explore_get()
    assert (got["env"] == 0).all() and (got["samples"] == 0).all() and np.isnan(got["leg_limits"]).all()
    e.record_start(fields=("drag", "solver"), every=1, capacity=K)
    seen = 0
    for n in (1, 1, K // 3, K - K // 3 - 2):                                                   # (read in the first periods, too)
        run_periods(e, n)
        seen += n
        rec, got = e.record_get(), e.explore_get()
        assert rec["idx"].shape == (B, seen) and rec["dropped"] == 0
        env, samples = envelope(rec, rules["mode"])
        assert np.array_equal(got["env"], env) and np.array_equal(got["samples"], samples), seen
    flights = (rec["idx"] == 0).sum(axis=1)
    print(f"envelope, mode {mode}: flights begun per quadrotor min {flights.min()} max {flights.max()}, samples {got['samples'].tolist()[:8]}, "
          f"largest reach {np.abs(got['env']).max():.3f} m/s")
    assert flights.min() >= 3 and np.abs(got["env"]).max() > 0.1                              # hover and two flights: the envelope restarted, or did not
    if mode == EXPLORE_CUMULATIVE:
        assert (got["samples"] == K).all()
    else:
        assert (got["samples"] < K).all() and (got["samples"] >= 1).all()
    e.close()


# ------------------------------------------------------------------ 3. bit identity with the host loop
def host_loop(e, legs, wp, rules, mask, K, x_meas=None):
    """The loop that exists without the feature.  Returns the mission log it implies, the limits it chose [B, L, 3] (NaN: none), what
    `explored` would have been over all three axes [B, L], and the last measurement."""
    B = legs.shape[0]
    log = dict(leg=np.zeros(B, np.int32), installed=np.zeros(B, np.int32), leg_code=np.full((B, L), REPLAN_SKIPPED, np.int32),
               leg_period=np.full((B, L), -1, np.int32))
    limits, all_axes = np.full((B, L, 3), np.nan), np.full((B, L), np.nan)
    rules7 = rules.copy()
    rules7["axes"] = 7
    leg, ar = log["leg"], np.arange(B)
    e.record_start(fields=("drag", "solver"), every=1, capacity=K)
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
        at = np.minimum(leg, L - 1)
        env, samples = envelope(e.record_get(), rules["mode"])
        explored, v, a = explore_velocity(env, samples, rules)
        now = legs[ar, at]
        chosen = due & (mask[ar, at] != 0)
        v_now, a_now = np.where(chosen, v, now["v_max"]), np.where(chosen, a, now["a_max"])
        sel = np.flatnonzero(chosen)
        limits[sel, leg[sel]] = np.stack([explored, v, a], axis=1)[sel]
        all_axes[sel, leg[sel]] = explore_velocity(env, samples, rules7)[0][sel]
        codes = np.full(B, REPLAN_SKIPPED, np.int32)
        circ = due & (now["kind"] == LEG_CIRCLE)
        if circ.any():
            c = e.replan_circle(np.where(circ, now["radius"], 1.0), v_now, "acc_dec", DT, start=start, mask=circ)
            codes[circ] = c[circ]
        way = due & (now["kind"] == LEG_WAYPOINTS)
        for vv, aa in sorted(set(zip(v_now[way].tolist(), a_now[way].tolist()))):
            m = way & (v_now == vv) & (a_now == aa)
            c = e.replan(wp[ar, at], vv, aa, DT, 4, start=start, mask=m)
            codes[m] = c[m]
        sel = np.flatnonzero(due)
        log["leg_code"][sel, leg[sel]] = codes[sel]
        log["leg_period"][sel, leg[sel]] = k
        log["installed"][sel] += codes[sel] == REPLAN_DONE
        leg[sel] += 1
    e.record_stop()
    return log, limits, all_axes, x_meas


def check_every_branch(B, rules, mask, log, limits, all_axes):
    """The window is not vacuous: asserted on the host loop alone."""
    step = rules["step"]
    kind = np.arange(B) % 5
    written = ~np.isnan(limits[:, :, 0])
    assert np.array_equal(written, (log["leg_period"] >= 0) & (mask != 0))
    assert log["installed"].min() >= 2, log["installed"]
    explored, v, a = limits[:, :, 0], limits[:, :, 1], limits[:, :, 2]
    nxt = explored + step[:, None]
    distinct = [len(np.unique(v[b][written[b]])) for b in np.flatnonzero(kind == 0)]
    print(f"host loop: installs per quadrotor min {log['installed'].min()} max {log['installed'].max()}; quadrotor 0 flew v_max {v[0].tolist()}; "
          f"distinct v_max of the quadrotors that always take explored + step: min {min(distinct)}; last leg consumed in period {log['leg_period'].max()}")
    assert min(distinct) >= 3
    for k, what in ((0, "explored + step"), (1, "desired"), (2, "v clipped"), (3, "a clipped only"), (4, "axes = 3")):
        w = written & (kind == k)[:, None]
        assert w.any() or B < 5, what
        if k == 0:
            ok = (v[w] == nxt[w]) & (a[w] == nxt[w]) & (nxt[w] < 50.0)
        elif k == 1:
            ok = (v[w] == (0.9 * step)[:, None].repeat(L, 1)[w]) & (a[w] == v[w]) & (nxt[w] >= v[w])
        elif k == 2:
            ok = (v[w] == (0.9 * step)[:, None].repeat(L, 1)[w]) & (a[w] == nxt[w]) & (a[w] > v[w])
        elif k == 3:
            ok = (a[w] == (0.8 * step)[:, None].repeat(L, 1)[w]) & (v[w] == nxt[w]) & (v[w] > a[w])
        else:
            ok = (v[w] == nxt[w])
            differs = int((explored[w] != all_axes[w]).sum())
            print(f"axes = 3: {differs} of {int(w.sum())} legs explored further than all three axes would have")
            assert differs >= 1 or B < 50                                                     # (one quadrotor of this kind on the emulator, fourteen on the GPU)
        print(f"{what}: {int(w.sum())} legs")
        assert ok.all(), what


def case_host_loop(lib, B, K, shape, step_path=False, fleet=False, circle=False, **cfg):
    x0, traj, lens, wp, legs = make_queue(B, shape, 83, circle=circle)
    rules, mask = make_rules(B, shape["step"]), make_mask(B)

    def engine():
        e = start_engine(lib, B, x0, traj, lens, **cfg)
        if fleet:
            e.fleet_set(fleet_sample(13, 0, B, e.cfg, spread=1.2, payload_max=0.05))
        return e
    a = engine()
    log, limits, all_axes, xa = host_loop(a, legs, wp, rules, mask, K, x_meas=x0.copy() if step_path else None)
    check_every_branch(B, rules, mask, log, limits, all_axes)
    b = engine()
    b.mission_set_legs(legs, wp, dt=DT)
    b.explore_start(rules, leg_mask=mask)
    xb = run_periods(b, K, x_meas=x0.copy() if step_path else None)
    assert_same(log, b.mission_get(), LOG_KEYS)
    got = b.explore_get()
    assert np.array_equal(got["leg_limits"], limits, equal_nan=True)
    assert_same(snapshot(a), snapshot(b))
    if step_path:
        assert np.array_equal(xa, xb)
    if circle:
        assert (log["leg_code"][:, 1] == REPLAN_DONE).all()
    a.close(); b.close()


# ------------------------------------------------------------------ 4. checkpoint
def case_checkpoint(lib, B, K0, K, shape):
    x0, traj, lens, wp, legs = make_queue(B, shape, 85)
    rules, mask = make_rules(B, shape["step"]), make_mask(B)
    e = start_engine(lib, B, x0, traj, lens)
    e.mission_set_legs(legs, wp, dt=DT)
    e.explore_start(rules, leg_mask=mask)
    run_periods(e, K0)
    leg, ex = e.mission_get()["leg"], e.explore_get()
    assert (leg >= 1).all() and (leg < L).all() and (ex["samples"] >= 1).all()
    st, sv, (x, _) = e.get_state(), e.get_solver_state(), e.sim_get_state()
    t, ln = e.get_trajectories()
    f = Engine(config(B), lib_path=lib)
    f.set_trajectories(t, ln)
    f.set_state(**st)
    f.set_solver_state(**sv)
    f.sim_reset(x)
    f.mission_set_legs(legs, wp, dt=DT, leg0=leg)
    f.explore_start(rules, leg_mask=mask, env=ex["env"], samples=ex["samples"])
    assert_same(ex, f.explore_get(), ("env", "samples"))
    run_periods(e, K); run_periods(f, K)
    assert_same(snapshot(e), snapshot(f))
    me, mf, ge, gf = e.mission_get(), f.mission_get(), e.explore_get(), f.explore_get()
    assert np.array_equal(me["leg"], mf["leg"]) and (me["leg"] > leg).all()
    assert_same(ge, gf, ("env", "samples"))
    new = mf["leg_period"] >= 0                        # the restored engine's logs hold what happened since
    assert np.array_equal(new, me["leg_period"] >= K0)
    assert np.array_equal(ge["leg_limits"][new], gf["leg_limits"][new], equal_nan=True) and np.isnan(gf["leg_limits"][~new]).all()
    assert (~np.isnan(gf["leg_limits"][new])).any()
    e.close(); f.close()


# ------------------------------------------------------------------ 5. off is the parent
def case_off_is_parent(lib, B, K, shape):
    x0, traj, lens, wp, legs = make_queue(B, shape, 87)
    runs = []
    for how in ("never", "stopped", "zero mask"):
        e = start_engine(lib, B, x0, traj, lens)
        e.mission_set_legs(legs, wp, dt=DT)
        if how == "stopped":
            e.explore_start(make_rules(B, shape["step"]))
            e.explore_stop()
            expect_rc(MPCQ_ERR_STATE, e.explore_stop)
        elif how == "zero mask":
            e.explore_start(make_rules(B, shape["step"], mode=EXPLORE_CUMULATIVE), leg_mask=np.zeros((B, L), np.uint8))
        run_periods(e, K, block=7)
        if how == "zero mask":
            got = e.explore_get()
            assert np.isnan(got["leg_limits"]).all() and (got["samples"] == K).all() and np.abs(got["env"]).max() > 0.1
        runs.append(dict(snapshot(e), **{k: v for k, v in e.mission_get().items() if k in LOG_KEYS}))
        e.close()
    assert runs[0]["installed"].min() >= 2
    assert_same(runs[0], runs[1])
    assert_same(runs[0], runs[2])


# ------------------------------------------------------------------ 6. state and argument rules
def case_rules(lib, B):
    x0, traj, lens, wp, legs = make_queue(B, EMU_SHAPE, 89, legs_n=1)
    e = start_engine(lib, B, x0, traj, lens)
    assert b"mpcq 0.6.7" in e.lib.mpcq_version()
    good = make_rules(B, 2.0)
    size = EXPLORE_RULE_DTYPE.itemsize
    ptr = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)

    def start(rules=good, rule_size=size, env=None, samples=None):
        return e.lib.mpcq_explore_start(e.h, ptr(rules), rule_size, None, _lib.d(env), _lib.l(samples))
    assert start() == MPCQ_ERR_STATE and "mission" in e.lib.mpcq_last_error().decode()        # no mission set
    with pytest.raises(_lib.MpcqError):
        e.explore_start(good)
    assert e.lib.mpcq_explore_get(e.h, None, None, None) == MPCQ_ERR_STATE
    assert e.lib.mpcq_explore_stop(e.h) == MPCQ_ERR_STATE
    e.mission_set_legs(legs, wp, dt=DT)
    assert e.lib.mpcq_explore_get(e.h, None, None, None) == MPCQ_ERR_STATE                    # a mission, but no exploration
    expect_rc(MPCQ_ERR_STATE, e.explore_get)

    def bad_calls():
        yield dict(rules=None), ("rules",)
        yield dict(rule_size=size - 8), ("rule_size",)
        yield dict(rule_size=size + 8), ("rule_size",)
        yield dict(env=np.zeros((B, 3, 2))), ("env0",)
        yield dict(samples=np.zeros(B, np.int64)), ("samples0",)
        neg = np.zeros(B, np.int64)
        neg[B - 1] = -1
        yield dict(env=np.zeros((B, 3, 2)), samples=neg), (f"quadrotor {B - 1}", "samples0")
        for name in ("step", "desired", "v_limit", "a_limit"):
            for v in (np.nan, np.inf, 0.0, -1.0):
                r = good.copy()
                b = B - 1 if name == "step" else 1
                r[name][b] = v
                yield dict(rules=r), (f"quadrotor {b}", name)
        for name, values in (("mode", (-1, 2)), ("axes", (0, 8, -1))):
            for v in values:
                r = good.copy()
                r[name][0] = v
                yield dict(rules=r), ("quadrotor 0", name)

    def refused(kw, names, running):
        before = snapshot(e), (e.explore_get() if running else None)
        assert start(**kw) == MPCQ_ERR_INVALID, kw
        msg = e.lib.mpcq_last_error().decode()
        for n in names:
            assert n in msg, (n, msg)
        assert_same(before[0], snapshot(e))
        if running:
            assert_same(before[1], e.explore_get())
        else:
            assert e.lib.mpcq_explore_stop(e.h) == MPCQ_ERR_STATE                             # the refused call started nothing
    calls = list(bad_calls())
    for kw, names in calls:
        refused(kw, names, running=False)
    e.explore_start(good)
    e.sim_steps(2, 2, 5e-3)
    got = e.explore_get()
    assert got["leg_limits"].shape == (B, 1, 3) and (got["samples"] >= 1).all()
    assert got["leg_limits"][:, 0, 0].tolist() == [0.0] * B                                   # hover: nothing explored, the first leg flies `step` (or its clip)
    assert np.array_equal(got["leg_limits"][:, 0, 1], explore_velocity(np.zeros((B, 3, 2)), np.zeros(B), good)[1])
    for kw, names in calls:
        refused(kw, names, running=True)
    expect_rc(MPCQ_ERR_STATE, e.sim_run, 2, 2, 5e-3)                                          # one persistent launch
    assert "explore" in e.lib.mpcq_last_error().decode()
    # calling start again replaces the rules (and empties envelope and log): the next leg written follows the new ones
    x0, traj, lens, wp, legs = make_queue(B, EMU_SHAPE, 90)
    e.set_trajectories(traj, lens)
    e.sim_reset(x0)
    e.mission_set_legs(legs, wp, dt=DT)                                                        # ends the exploration: its table is gone
    assert e.lib.mpcq_explore_stop(e.h) == MPCQ_ERR_STATE
    e.explore_start(explore_rules(B, step=2.0, desired=50.0))
    e.explore_start(explore_rules(B, step=3.5, desired=50.0, mode=EXPLORE_CUMULATIVE), env=np.tile([-1.0, 0.5], (B, 3, 1)), samples=np.full(B, 4))
    got = e.explore_get()
    assert (got["samples"] == 4).all() and np.isnan(got["leg_limits"]).all() and np.array_equal(got["env"], np.tile([-1.0, 0.5], (B, 3, 1)))
    e.sim_steps(1, 2, 5e-3)
    got = e.explore_get()
    assert (got["samples"] == 5).all() and (got["leg_limits"][:, 0] == [1.0, 4.5, 4.5]).all() and np.isnan(got["leg_limits"][:, 1:]).all()
    e.mission_stop()                                                                          # ends the exploration as well
    assert e.lib.mpcq_explore_get(e.h, None, None, None) == MPCQ_ERR_STATE
    assert e.lib.mpcq_explore_stop(e.h) == MPCQ_ERR_STATE
    e.sim_run(1, 2, 5e-3)                                                                     # legal again
    e.close()


# ------------------------------------------------------------------ lane emulator (CPU)
def test_emu_envelope_cumulative(emu):
    case_envelope(emu, 2, 170, EMU_SHAPE, EXPLORE_CUMULATIVE)


def test_emu_envelope_last_flight(emu):
    case_envelope(emu, 2, 170, EMU_SHAPE, EXPLORE_LAST_FLIGHT)


def test_emu_host_loop(emu):
    case_host_loop(emu, 5, 170, EMU_SHAPE)


def test_emu_host_loop_step_path(emu):
    case_host_loop(emu, 2, 165, EMU_SHAPE, step_path=True)


def test_emu_host_loop_fleet(emu):
    case_host_loop(emu, 2, 165, EMU_SHAPE, fleet=True)


def test_emu_host_loop_circle_leg(emu):
    case_host_loop(emu, 2, 165, EMU_SHAPE, circle=True)


def test_emu_checkpoint(emu):
    case_checkpoint(emu, 3, 40, 110, EMU_SHAPE)


def test_emu_off_is_parent(emu):
    case_off_is_parent(emu, 2, 150, EMU_SHAPE)


def test_emu_rules(emu):
    case_rules(emu, 4)


# ------------------------------------------------------------------ MI355X
gpu = pytest.mark.gpu
GPU_B, GPU_K = 70, 2300


@gpu
@pytest.mark.parametrize("mode", [EXPLORE_CUMULATIVE, EXPLORE_LAST_FLIGHT])
def test_gpu_envelope(mode):
    case_envelope(None, GPU_B, GPU_K, GPU_SHAPE, mode)


@gpu
def test_gpu_host_loop():
    case_host_loop(None, GPU_B, GPU_K, GPU_SHAPE)


@gpu
def test_gpu_host_loop_step_path():
    case_host_loop(None, GPU_B, GPU_K, GPU_SHAPE, step_path=True)


@gpu
def test_gpu_host_loop_fleet():
    case_host_loop(None, GPU_B, GPU_K, GPU_SHAPE, fleet=True)


@gpu
def test_gpu_host_loop_circle_leg():
    case_host_loop(None, GPU_B, GPU_K, GPU_SHAPE, circle=True)


@gpu
def test_gpu_host_loop_two_groups():
    case_host_loop(None, GPU_B, GPU_K, GPU_SHAPE, tune=dict(groups=2))


@gpu
def test_gpu_host_loop_f32():
    case_host_loop(None, GPU_B, GPU_K, GPU_SHAPE, precision=1)


@gpu
def test_gpu_checkpoint():
    case_checkpoint(None, GPU_B, 300, 1500, GPU_SHAPE)


@gpu
def test_gpu_off_is_parent():
    case_off_is_parent(None, GPU_B, 900, GPU_SHAPE)


@gpu
def test_gpu_rules():
    case_rules(None, GPU_B)

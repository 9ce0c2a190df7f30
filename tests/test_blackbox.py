"""The incident recorder (mpcq_blackbox_*, csrc/mpcq_blackbox.hpp) against the flight recorder that already exists, bit for bit, and the
host restatement of its rule (params.blackbox_causes).  The same cases run on the lane emulator (CPU, B = 3 .. 6; 24 where three groups are needed) and on the MI355X (-m gpu,
the product library).

The engine is deterministic, so the main case flies twice: run A records every watched quadrotor, the test reads thresholds off those rows
that put the incidents where it wants them (the midpoint of a step of the running maximum of err_pos^2 / speed^2 / cost, evaluated with
blackbox_causes' own expressions), and run B flies the same inputs with the recorder and the black box both on.  Nothing needs a tolerance.
One period is sim_steps(1, 2, 5e-3) (or one step(x_meas)); N = 10, nb = 10 everywhere."""
import os
import subprocess

import numpy as np
import pytest

from mpc_quad_ros_amd import _lib
from mpc_quad_ros_amd.engine import RECORD_DEFAULT, RECORD_FIELDS, Engine
from mpc_quad_ros_amd.logger import SwarmLogger
from mpc_quad_ros_amd.params import (BB_COST, BB_ERR_POS, BB_FALLBACK, BB_NONFINITE, BB_SPEED, BB_STATUS, BB_TILT, BLACKBOX_RULE_DTYPE,
                                     blackbox_causes, blackbox_rules, explore_rules, fleet_sample)
from mpc_quad_ros_amd.trajectories import mission_legs
from test_fleet import header_struct
from test_mission import DT, assert_same, expect_rc, start_engine, workload
from test_record import new_engine
from test_record import snapshot as full_snapshot

HERE = os.path.dirname(os.path.abspath(__file__))
EMU_DIR = os.path.join(HERE, "wave_emu")
EMU = os.path.join(EMU_DIR, "libmpcq_emu.so")
MPCQ_ERR_INVALID, MPCQ_ERR_STATE = -1, -3
MPCQ_SOLVE_NAN = 1
ALL = tuple(RECORD_FIELDS)
ROW_KEYS = ("x_odom", "x_ref", "w_odom", "x_pred_odom", "cost_solution", "v_body", "a_drag", "rgp_mu_g_t", "rgp_C_g_t", "status", "qp_iter",
            "idx", "finished")
INT_KEYS = ("status", "qp_iter", "idx", "finished")
INFO_KEYS = ("fired_period", "cause", "state", "rows", "fired_row")
L = 3


@pytest.fixture(scope="module")
def emu():
    subprocess.check_call(["make", "-C", EMU_DIR], stdout=subprocess.DEVNULL)
    return EMU


def fly(e, K, block=7):
    k = 0
    while k < K:
        n = min(block, K - k)
        e.sim_steps(n, 2, 5e-3)
        k += n


def sweep(lib, B, seed, size, Tmax, **cfg):
    """A mission of L legs per quadrotor (test_mission.workload) flown at limits that differ from quadrotor to quadrotor, some of them
    (from quadrotor 2 on) slow enough that their speed still rises at the end of the run: incidents everywhere between the first period
    and the last."""
    x0, traj, lens, wp = workload(B, L, 1, size, seed, Tmax=Tmax)
    v = np.full((B, 1), 12.0)
    slow = 2 if B < 14 else 10
    v[2:2 + slow, 0] = np.geomspace(0.3, 0.5 if B < 14 else 1.5, slow)
    e = start_engine(lib, B, x0, traj, lens, **cfg)
    e.mission_set_legs(mission_legs(B, L, v), wp, dt=DT)
    return e


def quantity(rec, name):
    """What a threshold cause compares, with blackbox_causes' expressions: [count, T]"""
    if name == "cost":
        return rec["cost_solution"]
    d = rec["x_odom"][:, :, 0:3] - rec["x_ref"][:, :, 0:3] if name == "err_pos" else rec["x_odom"][:, :, 7:10]
    return (d[:, :, 0] * d[:, :, 0] + d[:, :, 1] * d[:, :, 1]) + d[:, :, 2] * d[:, :, 2]


def threshold(q, lo, hi, squared):
    """(f, threshold): the last period f in [lo, hi] at which the running maximum of q [T] rises, and the threshold whose (square, if
    `squared`) is the midpoint of that rise -- q first exceeds it in period f.  None if the maximum does not rise in the window."""
    for f in range(min(hi, len(q) - 1), max(lo, 1) - 1, -1):
        before = q[:f].max()
        if q[f] > before:
            mid = 0.5 * (before + q[f])
            t = np.sqrt(mid) if squared else mid
            lim = t * t if squared else t
            if before < lim < q[f] and np.abs(q - lim).min() > 1e-9 * abs(lim):     # (nothing rests on a tie)
                return f, t
    return None


def expected(rec, rules, K, pre, post, D, p0=0):
    """What the black box must hold after periods p0 .. K - 1 of the recording `rec` (rows = periods): per quadrotor the firing period,
    cause, state, and the periods its ring holds."""
    c = blackbox_causes(rec, rules)[:, p0:]
    out = []
    for j in range(len(rules)):
        hit = np.flatnonzero(c[j])
        if len(hit):
            f = p0 + int(hit[0])
            lo, hi = max(p0, f - pre), min(K - 1, f + post)
            out.append(dict(f=f, cause=int(c[j, hit[0]]), state=2 if f + post <= K - 1 else 1, lo=lo, hi=hi, fired_row=f - lo))
        else:
            out.append(dict(f=-1, cause=0, state=0, lo=max(p0, K - D), hi=K - 1, fired_row=-1))
    return out


def check_box(box, rec, want, D, items=None):
    """The read-out `box` (blackbox_get) against rows of the recording `rec` and the expectation `want` (item i of the box is
    want[items[i]] and row items[i] of the recording)."""
    items = range(len(want)) if items is None else items
    assert len(box["rows"]) == len(items)
    for i, j in enumerate(items):
        w = want[j]
        n = w["hi"] - w["lo"] + 1
        assert (box["fired_period"][i], box["cause"][i], box["state"][i], box["rows"][i], box["fired_row"][i]) == \
            (w["f"], w["cause"], w["state"], n, w["fired_row"]), (j, w, {k: box[k][i] for k in INFO_KEYS})
        assert np.array_equal(box["period"][i, :n], np.arange(w["lo"], w["hi"] + 1)) and (box["period"][i, n:] == -1).all(), j
        for k in ROW_KEYS:
            if k not in box:
                continue
            assert np.array_equal(box[k][i, :n], rec[k][j, w["lo"]:w["hi"] + 1], equal_nan=True), (j, k)
            rest = box[k][i, n:]
            assert (rest == -1).all() if k in INT_KEYS else np.isnan(rest).all(), (j, k)


# ------------------------------------------------------------------ 1. the main case: two runs, the recorder as the yardstick
def case_main(lib, B, K, pre, post, size, Tmax, seed=41, **cfg):
    D = pre + 1 + post
    a = sweep(lib, B, seed, size, Tmax, **cfg)
    a.record_start(fields=ALL, capacity=K)
    fly(a, K)
    rec, snap_a = a.record_get(), full_snapshot(a)
    a.close()
    # the roles, each on a quadrotor of its own, and the thresholds that produce them, read off run A
    rules = blackbox_rules(B, nonfinite=True)
    names = {"err_pos": BB_ERR_POS, "speed": BB_SPEED, "cost": BB_COST}
    q = {n: quantity(rec, n) for n in names}
    roles = {"first": 0, "never": 1}
    rules[0]["causes"] |= BB_TILT | BB_COST
    rules[0]["tilt_cos"], rules[0]["cost"] = 2.0, -1.0
    windows = {"early": (1, pre - 1, ("err_pos", "speed", "cost")), "late": (K - post, K - 1, ("speed", "err_pos", "cost")),
               "wrapped": (2 * D, K - 1 - post, ("cost", "speed", "err_pos"))}
    free = list(range(2, B))
    planned = {}
    for role, (lo, hi, order) in windows.items():
        found = None
        for n in order:
            for j in free:
                th = threshold(q[n][j], lo, hi, n != "cost")
                if th is not None:
                    found = (j, n, th)
                    break
            if found:
                break
        assert found, f"run A shows no quadrotor for the role {role!r}"
        j, n, (f, t) = found
        free.remove(j)
        roles[role] = j
        rules[j]["causes"] |= names[n]
        rules[j][n] = t
        planned[j] = f
    for i, j in enumerate(free):             # everybody else: some incident anywhere, if the rows offer one
        n = ("speed", "err_pos", "cost")[i % 3]
        th = threshold(q[n][j], 1, K - 1 - (i % 2) * post, n != "cost")
        if th is not None:
            rules[j]["causes"] |= names[n]
            rules[j][n] = th[1]
            planned[j] = th[0]
    want = expected(rec, rules, K, pre, post, D)
    # the situations, on run A alone
    assert want[roles["first"]]["f"] == 0 and want[roles["first"]]["cause"] == BB_TILT | BB_COST
    assert want[roles["never"]]["f"] == -1
    assert 0 < want[roles["early"]]["f"] < pre
    assert want[roles["late"]]["f"] + post > K - 1 and want[roles["late"]]["state"] == 1
    assert want[roles["wrapped"]]["f"] >= 2 * D and want[roles["wrapped"]]["state"] == 2
    for j, f in planned.items():
        assert want[j]["f"] == f, (j, f, want[j])
    seen = 0
    for w in want:
        seen |= w["cause"]
    assert bin(seen).count("1") >= 3
    # run B
    b = sweep(lib, B, seed, size, Tmax, **cfg)
    b.record_start(fields=ALL, capacity=K)
    b.blackbox_start(rules, fields=ALL, pre=pre, post=post)
    fly(b, K)
    rec_b, snap_b = b.record_get(), full_snapshot(b)
    for k in ROW_KEYS + ("period",):
        assert np.array_equal(rec_b[k], rec[k], equal_nan=True), k
    assert_same(snap_a, snap_b)
    box = b.blackbox_get()
    assert b.blackbox_info()["periods"] == K and np.array_equal(box["quads"], np.arange(B))
    check_box(box, rec, want, D)
    # read-out of subsets, in the caller's order
    fired = np.flatnonzero(box["fired_period"] >= 0)
    sub = b.blackbox_get("fired")
    assert np.array_equal(sub["which"], fired)
    pick = np.array([roles["wrapped"], roles["first"], roles["never"]], np.int32)
    for part, idx in ((sub, fired), (b.blackbox_get(pick), pick)):
        for k in ROW_KEYS + INFO_KEYS + ("period", "quads"):
            assert np.array_equal(part[k], box[k][idx], equal_nan=True), k
    # an incident as a recording: the reference's log layout through the logger, unchanged
    i = int(np.flatnonzero(pick == roles["wrapped"])[0])
    one = Engine.blackbox_recording(b.blackbox_get(pick), i)
    w = want[roles["wrapped"]]
    assert np.array_equal(one["period"], np.arange(w["lo"], w["hi"] + 1)) and one["quads"][0] == roles["wrapped"]
    log = SwarmLogger.from_recording(b, one, 0.01, t_cpu=0.0).quad_log(0)
    assert np.array_equal(np.asarray(log["x_odom"]).reshape(-1, 13), rec["x_odom"][roles["wrapped"], w["lo"]:w["hi"] + 1])
    b.blackbox_stop()
    b.close()


# ------------------------------------------------------------------ 2. caller-owned measurement: a NaN from period k on
def case_nan_measurement(lib, B=3, K=9, k_nan=4, victim=1, pre=2, post=2):
    e = new_engine(lib, B)
    rules = blackbox_rules(B, status_mask=MPCQ_SOLVE_NAN, nonfinite=True)
    e.record_start(fields=RECORD_DEFAULT, capacity=K)
    e.blackbox_start(rules, pre=pre, post=post)
    x = e.sim_get_state()[0]
    for k in range(K):
        xm = x.copy()
        if k >= k_nan:
            xm[victim, 0] = np.nan
        _, xp = e.step(xm)
        x = np.where(np.isfinite(xp), xp, x)
    rec, box = e.record_get(), e.blackbox_get()
    want = expected(rec, rules, K, pre, post, pre + 1 + post)
    check_box(box, rec, want, pre + 1 + post)
    assert want[victim]["f"] == k_nan and want[victim]["cause"] == BB_STATUS | BB_NONFINITE and want[victim]["state"] == 2
    assert box["status"][victim, box["fired_row"][victim]] & MPCQ_SOLVE_NAN
    assert not (box["status"][victim, :box["fired_row"][victim]] & MPCQ_SOLVE_NAN).any()
    others = [j for j in range(B) if j != victim]
    assert (box["fired_period"][others] == -1).all() and (box["state"][others] == 0).all()
    e.close()


# ------------------------------------------------------------------ 3. rearm
def case_rearm(lib, B=4, K0=8, K=16, pre=2, post=2):
    """Everybody fires in period 0 (tilt_cos = 2 holds always) and is frozen after `post` more; the odd quadrotors are rearmed behind
    period K0 - 1, fire again in period K0 and hold a second incident that begins there.  The others keep theirs byte for byte."""
    D = pre + 1 + post
    e = new_engine(lib, B)
    rules = blackbox_rules(B, tilt_cos=2.0)
    e.record_start(fields=ALL, capacity=K)
    e.blackbox_start(rules, fields=ALL, pre=pre, post=post)
    fly(e, K0, block=3)
    first = e.blackbox_get()
    assert (first["state"] == 2).all() and (first["fired_period"] == 0).all() and (first["rows"] == post + 1).all()
    mask = np.arange(B) % 2
    e.blackbox_rearm(mask)
    armed = e.blackbox_info()
    assert np.array_equal(armed["state"], np.where(mask, 0, 2)) and np.array_equal(armed["rows"], np.where(mask, 0, post + 1))
    assert np.array_equal(armed["fired_period"], np.where(mask, -1, 0)) and np.array_equal(armed["cause"], np.where(mask, 0, BB_TILT))
    fly(e, K - K0, block=3)
    rec, box = e.record_get(), e.blackbox_get()
    again, kept = np.flatnonzero(mask), np.flatnonzero(mask == 0)
    want = expected(rec, rules, K, pre, post, D, p0=K0)
    check_box(b_sub(box, again), rec, want, D, items=again)
    assert (box["fired_period"][again] == K0).all() and (box["period"][again, 0] == K0).all()
    for k in box:
        assert np.array_equal(box[k][kept], first[k][kept], equal_nan=True), k
    e.blackbox_rearm()                                       # everybody: empty rings
    info = e.blackbox_info()
    assert (info["state"] == 0).all() and (info["rows"] == 0).all() and (info["fired_period"] == -1).all()
    empty = e.blackbox_get()
    assert np.isnan(empty["x_odom"]).all() and (empty["period"] == -1).all() and (empty["status"] == -1).all()
    e.close()


def b_sub(box, idx):
    return {k: v[idx] for k, v in box.items()}


# ------------------------------------------------------------------ 4. selection across groups, in the caller's order
def case_selection(lib, B, K, quads, groups, pre=3, post=2):
    """An unsorted selection that spans the groups, with rules that differ per quadrotor: the same with every number of groups, and what
    the recorder's rows of the same run say."""
    D = pre + 1 + post
    quads = np.asarray(quads, np.int32)
    n = len(quads)
    i = np.arange(n)
    rules = blackbox_rules(n, fallback=i % 2 == 0, status_mask=-1, err_pos=np.where(i % 3 != 2, 0.005 + 0.01 * (i % 5), np.nan),
                           speed=np.where(i % 3 == 2, 0.1 + 0.03 * (i % 4), np.nan))
    boxes = []
    for g in groups:
        e = new_engine(lib, B, tune=dict(groups=g), seed=3)
        assert e.get_groups() == g
        e.record_start(quads=quads, fields=RECORD_DEFAULT, capacity=K)
        e.blackbox_start(rules, quads=quads, pre=pre, post=post)
        fly(e, K, block=4)
        rec, box = e.record_get(), e.blackbox_get()
        assert np.array_equal(box["quads"], quads)
        want = expected(rec, rules, K, pre, post, D)
        check_box(box, rec, want, D)
        assert len({w["f"] for w in want}) >= 3              # (the rules do differ in effect)
        which = np.arange(n - 1, -1, -2, dtype=np.int32)
        part = e.blackbox_get(which)
        for k in ROW_KEYS + INFO_KEYS + ("period", "quads"):
            if k in box:
                assert np.array_equal(part[k], box[k][which], equal_nan=True), k
        boxes.append(box)
        e.close()
    for box in boxes[1:]:
        for k in boxes[0]:
            assert np.array_equal(box[k], boxes[0][k], equal_nan=True), k


# ------------------------------------------------------------------ 5. next to mission + score + exploration + fleet
def case_coexistence(lib, B, K, size, Tmax):
    """The fleet sweep of INTEGRATION.md at test size, with the black box on and off: everything the other features report is the same."""
    x0, traj, lens, wp = workload(B, L, 1, size, 57, Tmax=Tmax)
    legs = mission_legs(B, L, np.linspace(3.0, 12.0, B)[:, None])
    out = []
    for on in (False, True):
        e = start_engine(lib, B, x0, traj, lens)
        e.fleet_set(fleet_sample(13, 0, B, e.cfg, spread=1.2, payload_max=0.05))
        e.mission_set_legs(legs, wp, dt=DT)
        e.explore_start(explore_rules(B, step=3.0))
        e.score_start(L + 1, tail_rows=10)
        if on:
            rules = blackbox_rules(B, status_mask=-1, fallback=True, err_pos=0.05, speed=1.0, tilt_cos=np.cos(0.3))
            e.blackbox_start(rules, pre=4, post=3)
            expect_rc(MPCQ_ERR_STATE, e.sim_run, 1, 2, 5e-3)
        fly(e, K)
        got = dict(full_snapshot(e))
        got.update({f"m_{k}": v for k, v in e.mission_get().items()})
        got.update({f"s_{k}": v for k, v in e.score_get().items()})
        got.update({f"e_{k}": v for k, v in e.explore_get().items()})
        if on:
            info = e.blackbox_info()
            assert info["periods"] == K and (info["fired_period"] >= 0).any()
        out.append(got)
        e.close()
    assert out[0]["m_installed"].min() >= 1
    assert_same(out[0], out[1])


# ------------------------------------------------------------------ 6. MPCQ_PRECISION_F32: the RGP rows are the recorder's
def case_f32(lib, B, K, pre=2, post=1):
    D = pre + 1 + post
    e = new_engine(lib, B, precision=1)
    rules = blackbox_rules(B, speed=np.where(np.arange(B) % 2 == 0, 0.03, np.nan))
    e.record_start(fields=ALL, capacity=K)
    e.blackbox_start(rules, fields=ALL, pre=pre, post=post)
    fly(e, K)
    rec, box = e.record_get(), e.blackbox_get()
    want = expected(rec, rules, K, pre, post, D)
    check_box(box, rec, want, D)
    assert any(w["f"] >= 0 for w in want) and np.abs(box["rgp_mu_g_t"][np.isfinite(box["rgp_mu_g_t"])]).max() > 0
    assert np.array_equal(box["rgp_mu_g_t"][np.isfinite(box["rgp_mu_g_t"])].astype(np.float32).astype(np.float64),
                          box["rgp_mu_g_t"][np.isfinite(box["rgp_mu_g_t"])])
    e.close()


# ------------------------------------------------------------------ 7. every refusal, and the engine left as it was
def case_errors(lib, B=4):
    e = new_engine(lib, B)
    lib_ = e.lib
    good = blackbox_rules(B, speed=0.03)

    def refused(rc, text, fn, *args, **kw):
        expect_rc(rc, fn, *args, **kw)
        assert text in lib_.mpcq_last_error().decode(), (text, lib_.mpcq_last_error().decode())
    for call in (e.blackbox_info, e.blackbox_get, e.blackbox_rearm, e.blackbox_stop):
        with pytest.raises(_lib.MpcqError):
            call()
    rc_none = (("mpcq_blackbox_info", lambda: lib_.mpcq_blackbox_info(e.h, None, None, None, None, None, None)),
               ("mpcq_blackbox_get", lambda: lib_.mpcq_blackbox_get(e.h, 1, None, 0, None)),
               ("mpcq_blackbox_get_solver", lambda: lib_.mpcq_blackbox_get_solver(e.h, None, 0, None)),
               ("mpcq_blackbox_get_periods", lambda: lib_.mpcq_blackbox_get_periods(e.h, None, 0, None)),
               ("mpcq_blackbox_rearm", lambda: lib_.mpcq_blackbox_rearm(e.h, None)),
               ("mpcq_blackbox_stop", lambda: lib_.mpcq_blackbox_stop(e.h)))
    for name, call in rc_none:
        assert call() == MPCQ_ERR_STATE and name in lib_.mpcq_last_error().decode(), name

    def rule(**kw):
        r = good.copy()
        for k, v in kw.items():
            r[k][2] = v
        return r
    table = [
        (dict(rules=good, fields=()), "fields"),
        (dict(rules=good, pre=-1), "pre and post"),
        (dict(rules=good, post=-1), "pre and post"),
        (dict(rules=good, pre=65000, post=536), "65536"),
        (dict(rules=good[:2], quads=[0, B]), "out of range"),
        (dict(rules=good[:2], quads=[-1, 0]), "out of range"),
        (dict(rules=good[:2], quads=[1, 1]), "duplicate"),
        (dict(rules=rule(causes=128 | BB_SPEED)), "quadrotor 2: causes"),
        (dict(rules=rule(speed=np.nan)), "quadrotor 2: speed"),
        (dict(rules=rule(causes=BB_ERR_POS, err_pos=np.nan)), "quadrotor 2: err_pos"),
        (dict(rules=rule(causes=BB_TILT, tilt_cos=np.nan)), "quadrotor 2: tilt_cos"),
        (dict(rules=rule(causes=BB_COST, cost=np.nan)), "quadrotor 2: cost"),
        (dict(rules=rule(err_pos=-0.5)), "quadrotor 2: err_pos"),
        (dict(rules=rule(speed=-1.0)), "quadrotor 2: speed"),
    ]
    for kw, text in table:
        refused(MPCQ_ERR_INVALID, text, e.blackbox_start, **kw)
        assert lib_.mpcq_blackbox_stop(e.h) == MPCQ_ERR_STATE             # nothing was started
    assert lib_.mpcq_blackbox_start(e.h, None, 0, 1 << 9, 1, 1, good.ctypes.data) == MPCQ_ERR_INVALID     # an unknown field bit
    assert lib_.mpcq_blackbox_start(e.h, None, 0, 1, 1, 1, None) == MPCQ_ERR_INVALID
    # a quadrotor named by its index, not by its place in the selection
    refused(MPCQ_ERR_INVALID, "quadrotor 3: speed", e.blackbox_start, rule(speed=-1.0)[1:3], quads=[0, 3])
    # a disabled cause's NaN threshold is not read
    off = good.copy()
    off["tilt_cos"], off["cost"] = np.nan, np.nan
    off = off[:3]
    e.blackbox_start(off, quads=[2, 0, 3], fields=("x_odom", "solver"), pre=1, post=1)
    refused(MPCQ_ERR_STATE, "running", e.blackbox_start, good)
    refused(MPCQ_ERR_STATE, "black box", e.sim_run, 1, 2, 5e-3)
    refused(MPCQ_ERR_INVALID, "outside the selection", e.blackbox_get, [0, 3])
    refused(MPCQ_ERR_INVALID, "outside the selection", e.blackbox_get, [-1])
    refused(MPCQ_ERR_INVALID, "duplicate", e.blackbox_get, [1, 1])
    out = np.zeros((3, 3, 13))
    assert lib_.mpcq_blackbox_get(e.h, RECORD_FIELDS["w_odom"], None, 0, _lib.d(out)) == MPCQ_ERR_INVALID      # not a field of this box
    assert lib_.mpcq_blackbox_get(e.h, RECORD_FIELDS["solver"], None, 0, _lib.d(out)) == MPCQ_ERR_INVALID
    assert lib_.mpcq_blackbox_get(e.h, 3, None, 0, _lib.d(out)) == MPCQ_ERR_INVALID
    # after the refusals: the box that was started works as if they had not been made
    e.record_start(quads=[2, 0, 3], fields=("x_odom", "x_ref", "w_odom", "cost_solution", "solver"), capacity=6)
    fly(e, 6)
    rec, box = e.record_get(), e.blackbox_get()
    assert set(box) & set(ROW_KEYS) == {"x_odom", "status", "qp_iter", "idx", "finished"} and np.array_equal(box["quads"], [2, 0, 3])
    check_box(box, rec, expected(rec, off, 6, 1, 1, 3), 3)
    e.blackbox_stop()
    expect_rc(MPCQ_ERR_STATE, e.blackbox_stop)
    e.blackbox_start(good)                                   # and a new one may start
    e.blackbox_stop()
    e.close()
    # an RGP field on an engine without RGP
    z = new_engine(lib, 2, nb=0)
    with pytest.raises(_lib.MpcqError, match="mpcq error -1:.*nb = 0"):
        z.blackbox_start(blackbox_rules(2), fields=("x_odom", "rgp_mu"))
    z.blackbox_start(blackbox_rules(2))                      # the default drops the RGP fields
    assert "rgp_mu_g_t" not in z.blackbox_get()
    z.close()


# ------------------------------------------------------------------ 8. no perturbation at B = 8 192, every quadrotor watched
def case_large(B=8192, K=40, pre=10, post=5):
    out = []
    for on in (False, True):
        e = new_engine(None, B, N=20, tune=dict(groups=2), seed=5)
        e.record_start(quads=np.arange(0, B, 128), fields=RECORD_DEFAULT, capacity=K)
        if on:
            rules = blackbox_rules(B, fallback=True, status_mask=-1, speed=0.02 + 0.1 * (np.arange(B) % 7))
            e.blackbox_start(rules, pre=pre, post=post)
        fly(e, K, block=20)
        got = dict(full_snapshot(e))
        got.update({f"r_{k}": v for k, v in e.record_get().items()})
        if on:
            info = e.blackbox_info()
            fired = np.flatnonzero(info["fired_period"] >= 0)
            assert len(fired) > B // 7 and info["periods"] == K
            sel = np.arange(0, B, 128, dtype=np.int32)
            box = e.blackbox_get(sel)                          # 64 rings travel, not 8 192
            rec = e.record_get()
            want = expected(rec, rules[sel], K, pre, post, pre + 1 + post)
            check_box(box, rec, want, pre + 1 + post)
        out.append(got)
        e.close()
    assert_same(out[0], out[1])


# ------------------------------------------------------------------ no library: the ABI struct and the host rule
def test_rule_dtype_matches_header():
    sizes = {"double": (8, np.float64), "int32_t": (4, np.int32)}
    fields = header_struct("mpcq_blackbox_rule")
    assert [f[0] for f in fields] == list(BLACKBOX_RULE_DTYPE.names)
    off = align = 0
    for name, ctype, count in fields:
        size, dt = sizes[ctype]
        off = (off + size - 1) // size * size
        assert BLACKBOX_RULE_DTYPE.fields[name][1] == off and BLACKBOX_RULE_DTYPE.fields[name][0].base == dt and count == 1, name
        off += size
        align = max(align, size)
    assert BLACKBOX_RULE_DTYPE.itemsize == (off + align - 1) // align * align == 40
    with open(os.path.join(HERE, "..", "include", "mpcq.h")) as fh:
        text = fh.read()
    for name, bit in (("STATUS", BB_STATUS), ("FALLBACK", BB_FALLBACK), ("NONFINITE", BB_NONFINITE), ("ERR_POS", BB_ERR_POS), ("SPEED", BB_SPEED),
                      ("TILT", BB_TILT), ("COST", BB_COST)):
        assert f"#define MPCQ_BB_{name}".ljust(25) in text and int(text.split(f"#define MPCQ_BB_{name}")[1].split()[0]) == bit


def test_host_rule_every_cause():
    """blackbox_causes on hand-made rows: every cause alone, all together, a NaN operand, and the strict inequalities at equality."""
    hover = np.array([0, 0, 3.0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0])
    T = 12
    x = np.tile(hover, (1, T, 1))
    ref = x.copy()
    w, cost = np.full((1, T, 4), 0.5), np.full((1, T), 1.0)
    status, it = np.zeros((1, T), np.int32), np.full((1, T), 3, np.int32)
    status[0, 1] = 4                       # 1: status (bit 4 of the mask 6)
    status[0, 11] = 1                      # (a status bit outside the mask)
    it[0, 2] = 1005                        # 2: fallback
    w[0, 3, 2] = np.inf                    # 3: non-finite control
    x[0, 4, 0:3] += [0.3, 0.4, 1.2]        # 4: err_pos 1.3 > 1
    x[0, 5, 7:10] = [2.0, 3.0, 6.0]        # 5: speed 7 > 5
    x[0, 6, 4] = 0.6                       # 6: 1 - 2 * 0.36 = 0.28 < 0.5
    cost[0, 7] = 10.5                      # 7: cost > 10
    # 8: all together
    status[0, 8], it[0, 8], x[0, 8, 0:3], x[0, 8, 7:10], x[0, 8, 4], cost[0, 8] = 2, 2001, ref[0, 8, 0:3] + [0, 0, 2], [0, 0, 6], 0.8, np.inf
    # 9: equality everywhere -- strict inequalities do not fire
    x[0, 9, 0:3] += [0, 0, 1.0]
    x[0, 9, 7:10] = [3.0, 4.0, 0.0]
    x[0, 9, 4], cost[0, 9] = 0.5, 10.0     # 1 - 2 * 0.25 = 0.5 exactly
    # 10: NaN operands -- every comparison false, NONFINITE raised
    x[0, 10, 2], x[0, 10, 9], x[0, 10, 4], cost[0, 10] = np.nan, np.nan, np.nan, np.nan
    rows = dict(x_odom=x, x_ref=ref, w_odom=w, cost_solution=cost, status=status, qp_iter=it)
    rules = blackbox_rules(1, status_mask=6, fallback=True, nonfinite=True, err_pos=1.0, speed=5.0, tilt_cos=0.5, cost=10.0)
    assert rules["causes"][0] == 127
    every = BB_STATUS | BB_FALLBACK | BB_NONFINITE | BB_ERR_POS | BB_SPEED | BB_TILT | BB_COST
    want = [0, BB_STATUS, BB_FALLBACK, BB_NONFINITE, BB_ERR_POS, BB_SPEED, BB_TILT, BB_COST, every, 0, BB_NONFINITE, 0]
    got = blackbox_causes(rows, rules)
    assert got.dtype == np.int32 and got.shape == (1, T) and got[0].tolist() == want
    # a cause that is not enabled is never raised; None / NaN switch a threshold cause off
    only = blackbox_rules(1, nonfinite=False, speed=5.0, cost=np.nan)
    assert only["causes"][0] == BB_SPEED
    assert blackbox_causes(rows, only)[0].tolist() == [0, 0, 0, 0, 0, BB_SPEED, 0, 0, BB_SPEED, 0, 0, 0]
    assert blackbox_causes(dict(x_odom=x), only)[0, 5] == BB_SPEED       # (only the rows an enabled cause reads are needed)
    with pytest.raises(ValueError):
        blackbox_causes(dict(x_odom=x), rules)
    # per-quadrotor arguments
    two = blackbox_rules(2, err_pos=[1.0, np.nan], fallback=[False, True], nonfinite=False)
    assert two["causes"].tolist() == [BB_ERR_POS, BB_FALLBACK]
    both = blackbox_causes({k: np.repeat(v, 2, axis=0) for k, v in rows.items()}, two)
    assert both[0].tolist() == [0, 0, 0, 0, BB_ERR_POS, 0, 0, 0, BB_ERR_POS, 0, 0, 0]
    assert both[1].tolist() == [0, 0, BB_FALLBACK, 0, 0, 0, 0, 0, BB_FALLBACK, 0, 0, 0]


# ------------------------------------------------------------------ lane emulator (CPU)
EMU_MAIN = dict(B=5, K=60, pre=5, post=3, size=0.3, Tmax=400)


def test_emu_main(emu):
    case_main(emu, **EMU_MAIN)


def test_emu_nan_measurement(emu):
    case_nan_measurement(emu)


def test_emu_rearm(emu):
    case_rearm(emu)


def test_emu_selection_across_groups(emu):
    case_selection(emu, 24, 8, [23, 0, 8, 7, 16, 15, 9], (1, 3))      # (a group holds at least 8 quadrotors: three groups of 8)


def test_emu_coexistence(emu):
    case_coexistence(emu, 3, 30, 0.3, 400)


def test_emu_f32(emu):
    case_f32(emu, 3, 8)


def test_emu_errors(emu):
    case_errors(emu)


# ------------------------------------------------------------------ MI355X
gpu = pytest.mark.gpu
GPU_MAIN = dict(B=70, K=300, pre=20, post=10, size=1.5, Tmax=2400)


@gpu
def test_gpu_main():
    case_main(None, **GPU_MAIN)


@gpu
def test_gpu_main_two_groups_f32():
    case_main(None, **GPU_MAIN, precision=1, tune=dict(groups=2))


@gpu
def test_gpu_rearm():
    case_rearm(None, B=70, K0=40, K=90, pre=20, post=10)


@gpu
def test_gpu_selection_across_groups():
    quads = [69, 0, 23, 24, 46, 47, 22, 45, 68, 1, 35]          # both sides of every boundary of three groups of 70
    case_selection(None, 70, 60, quads, (1, 3), pre=20, post=10)


@gpu
def test_gpu_coexistence():
    case_coexistence(None, 70, 300, 1.5, 2400)


@gpu
def test_gpu_f32():
    case_f32(None, 70, 40, pre=20, post=10)


@gpu
def test_gpu_errors():
    case_errors(None)


@gpu
def test_gpu_no_perturbation_b8192():
    case_large()

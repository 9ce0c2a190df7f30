"""The flight scoreboard (mpcq_score_start / _get, Engine.score_* and mission_scores): every period folded on the device into the row of
the flight the quadrotor is flying.  The same cases run on the lane emulator (CPU, B = 8) and on the MI355X (-m gpu, the product library).

The yardstick is the flight recorder of the same run (fields x_odom, x_ref, cost, solver; every period of every quadrotor): the table is
recomputed in numpy from its rows with the rules of include/mpcq.h -- a slot opens on a recorded cursor 0 when the current slot holds a
period, a period is a tail period iff cursor >= len - tail_rows, with len the length at that period (read in front of every period of
the base run, in front of every block where no mission changes it).
 * Counts, first_period, last_period, rows, finished, flights and overflow are equal.
 * Fields 1..7 are within rtol = 1e-12 (sum_cost: relative to sum |cost|): a sequential sum of n <= ~1 500 non-negative terms carries at
   most (n + 2) 2^-53 ~ 1.7e-13 relative error and a contracted multiply-add moves a term by one rounding; no flight here is longer.
Runs are made once per library and shared between the tests that compare them.
Out of bounds: the overflow case compares flights / overflow and the engine's whole state next to the table.  The emulator's `checked`
build was not run on these cases: it has to be loaded into python with the UBSan runtime preloaded, and score_kernel indexes through plain
pointers, which that build's region-checked pointers do not cover."""
import os
import subprocess

import numpy as np
import pytest

from mpc_quad_ros_amd import _lib
from mpc_quad_ros_amd.engine import LEG_CIRCLE, LEG_WAYPOINTS, REPLAN_DONE, REPLAN_TOO_LONG, SCORE_DERIVED, SCORE_FIELDS, SCORE_INT, Engine
from mpc_quad_ros_amd.trajectories import mission_legs
from test_circle_mission import DT, assert_same, expect_rc, hover_slots, snapshot, start_engine

HERE = os.path.dirname(os.path.abspath(__file__))
EMU_DIR = os.path.join(HERE, "wave_emu")
EMU = os.path.join(EMU_DIR, "libmpcq_emu.so")
MPCQ_ERR_INVALID, MPCQ_ERR_STATE = -1, -3
RTOL = 1e-12
L = 3
REC_FIELDS = ("x_odom", "x_ref", "cost_solution", "solver")
REC_KEYS = ("x_odom", "x_ref", "cost_solution", "status", "qp_iter", "idx", "finished", "period")


@pytest.fixture(scope="module")
def emu():
    subprocess.check_call(["make", "-C", EMU_DIR], stdout=subprocess.DEVNULL)
    return EMU


class Shape:
    """One sweep: B quadrotors, L = 3 legs, circle and waypoint legs mixed, v_max varying across the quadrotors, K periods.  The flights
    grow with the quadrotor's index (radius and waypoint spread times 0.02 .. 1), so within K periods the first quadrotors have flown
    all their legs and hold while the last are in mid-flight.  Quadrotor 0's second leg is a circle that does not fit Tmax."""

    def __init__(self, B, K, radii, speeds, size, Tmax, block, R):
        self.B, self.K, self.radii, self.speeds, self.size, self.Tmax, self.block, self.R = B, K, radii, speeds, size, Tmax, block, R


# the largest flights: ~80 rows on the emulator, a few hundred rows (radius 2.5 circles at 10 .. 15 m/s, waypoint legs under high limits) on the GPU
EMU_SHAPE = Shape(8, 48, (0.15, 0.2, 0.3), (5.0, 15.0), 0.5, 300, 11, 10)
EMU_GROUPS_SHAPE = Shape(16, 24, (0.15, 0.2, 0.3), (5.0, 15.0), 0.5, 300, 7, 10)   # two groups of 8
GPU_SHAPE = Shape(256, 300, (1.0, 2.5), (10.0, 15.0), 1.5, 600, 64, 60)


def sweep(sh, seed=71):
    rng = np.random.default_rng(seed)
    B = sh.B
    x0, traj, lens = hover_slots(B, sh.Tmax, seed + 100)
    kind = ((np.arange(B)[:, None] + np.arange(L)[None, :]) % 2).astype(np.int32)            # circle and waypoint legs alternate
    v = np.linspace(sh.speeds[0], sh.speeds[1], B)[:, None] * np.ones((1, L))                # the sweep: v_max across the quadrotors
    scale = 0.02 + 0.98 * np.linspace(0.0, 1.0, B) ** 2
    legs = mission_legs(B, L, v, a_max=40.0, kind=kind, radius=rng.choice(sh.radii, (B, L)) * scale[:, None])
    wp = x0[:, None, None, 0:3] + rng.uniform(-sh.size, sh.size, (B, L, 2, 3)) * scale[:, None, None, None]
    legs["kind"][0, 1], legs["radius"][0, 1] = LEG_CIRCLE, 40.0   # 4 pi 40 / v / dt rows do not fit Tmax: REPLAN_TOO_LONG
    return x0, traj, lens, legs, wp


def lengths(e):
    ln = np.zeros(e.B, np.int32)
    e._check(e.lib.mpcq_get_trajectories(e.h, None, _lib.i(ln)))
    return ln


# ------------------------------------------------------------------ the yardstick
def table_from_rows(rec, len_hist, F, tail_rows):
    """(table [B,F,16], flights [B], overflow [B], sum |cost| [B,F]) from the recorder's rows and the lengths [T,B] at every period."""
    B, T = rec["idx"].shape
    tab = np.zeros((B, F, 16))
    tab[:, :, 12:14] = -1
    abs_cost = np.zeros((B, F))
    cur, overflow, used, ar = np.zeros(B, np.int64), np.zeros(B, np.int64), np.zeros(B, np.int64), np.arange(B)
    for p in range(T):
        i, ln = rec["idx"][:, p].astype(np.int64), len_hist[p].astype(np.int64)
        c = np.minimum(cur, F - 1)
        cur += (i == 0) & (cur < F) & (tab[ar, c, 0] + tab[ar, c, 8] > 0)
        ok = cur < F
        overflow += ~ok
        s = np.flatnonzero(ok)
        c = cur[s]
        used[s] = c + 1
        x, r = rec["x_odom"][s, p], rec["x_ref"][s, p]
        ep, ev = ((x[:, 0:3] - r[:, 0:3]) ** 2).sum(axis=1), ((x[:, 7:10] - r[:, 7:10]) ** 2).sum(axis=1)
        v2, vr2 = (x[:, 7:10] ** 2).sum(axis=1), (r[:, 7:10] ** 2).sum(axis=1)
        cost, it = rec["cost_solution"][s, p], rec["qp_iter"][s, p].astype(np.int64)
        nt = (i[s] < ln[s] - tail_rows).astype(np.float64)      # 1: not a tail period
        tab[s, c, 0] += nt
        tab[s, c, 1] += nt * ep
        tab[s, c, 2] += nt * ev
        tab[s, c, 3] = np.where(nt > 0, np.maximum(tab[s, c, 3], ep), tab[s, c, 3])
        tab[s, c, 4] += nt * np.sqrt(ep / 3.0)
        tab[s, c, 5] = np.where(nt > 0, np.maximum(tab[s, c, 5], v2), tab[s, c, 5])
        tab[s, c, 6] = np.where(nt > 0, np.maximum(tab[s, c, 6], vr2), tab[s, c, 6])
        tab[s, c, 7] += nt * cost
        abs_cost[s, c] += nt * np.abs(cost)
        tab[s, c, 8] += 1 - nt
        tab[s, c, 9] += rec["status"][s, p] != 0
        tab[s, c, 10] += (it // 1000) % 10 != 0
        tab[s, c, 11] += it % 1000
        tab[s, c, 12] = np.where(tab[s, c, 12] < 0, p, tab[s, c, 12])
        tab[s, c, 13] = p
        tab[s, c, 14] = ln[s]
        tab[s, c, 15] = np.maximum(tab[s, c, 15], rec["finished"][s, p] != 0)
    return tab, used, overflow, abs_cost


def assert_table(run, len_hist, what):
    """The scoreboard of a run against the table recomputed from the recorder of the same run."""
    sc, rec = run["score"], run["rec"]
    assert rec["dropped"] == 0 and rec["period"].tolist() == list(range(run["K"]))
    want, used, overflow, abs_cost = table_from_rows(rec, len_hist, run["F"], run["tail_rows"])
    assert sc["periods"] == run["K"]
    assert np.array_equal(sc["flights"], used), what
    assert np.array_equal(sc["overflow"], overflow), what
    for k, name in enumerate(SCORE_FIELDS):
        got = sc[name]
        if k in SCORE_INT:
            assert got.dtype == np.int64 and np.array_equal(got, want[:, :, k].astype(np.int64)), (what, name)
            continue
        scale = abs_cost if name == "sum_cost" else np.abs(want[:, :, k])
        err = np.abs(got - want[:, :, k])
        worst = (err / np.where(scale > 0, scale, 1.0)).max()
        print(f"{what}: {name} largest relative difference {worst:.3e} (largest value {np.abs(want[:, :, k]).max():.4g})")
        assert (err <= RTOL * scale).all(), (what, name, worst)
    total = (sc["steps"] + sc["tail_steps"]).sum(axis=1) + sc["overflow"]
    assert (total == sc["periods"]).all(), what                  # every period is in exactly one slot, or counted as overflow
    n = np.where(sc["steps"] > 0, sc["steps"], np.nan)
    for name, val in (("rmse_pos", np.sqrt(sc["sum_epos2"] / n)), ("mean_rms_pos", sc["sum_rms_pos"] / n),
                      ("peak_speed", np.where(sc["steps"] > 0, np.sqrt(sc["max_v2"]), np.nan))):
        assert np.array_equal(sc[name], val, equal_nan=True) and (np.isnan(sc[name]) == (sc["steps"] == 0)).all(), name
    return want


# ------------------------------------------------------------------ the runs
_RUNS = {}


def mission_run(lib, sh, F=4, tail_rows=0, block=None, path="sim", score=True, more=0, **cfg):
    """One mission sweep under the recorder (and the scoreboard).  path 'sim': sim_steps in blocks of `block` periods (1: the lengths
    in front of every period are logged); 'step': step(x_meas) with the host driving the plant (sim_plant_period)."""
    key = (lib, sh.B, F, tail_rows, block, path, score, more, tuple(sorted((k, repr(v)) for k, v in cfg.items())))
    if key in _RUNS:
        return _RUNS[key]
    B, K = sh.B, sh.K
    x0, traj, lens, legs, wp = sweep(sh)
    e = start_engine(lib, B, x0, traj, lens, **cfg)
    e.mission_set_legs(legs, wp, dt=DT)
    if score:
        e.score_start(F, tail_rows)
    e.record_start(fields=REC_FIELDS, every=1, capacity=K)
    len_hist = []
    if path == "step":
        x = x0.copy()
        for _ in range(K):
            len_hist.append(lengths(e))
            w, _ = e.step(x)
            e.sim_plant_period(w, 0.01, 5e-3)
            x = e.sim_get_state()[0]
    else:
        k = 0
        while k < K:
            n = min(block or sh.block, K - k)
            if n == 1:
                len_hist.append(lengths(e))
            e.sim_steps(n, 2, 5e-3)
            k += n
    run = dict(K=K, F=F, tail_rows=tail_rows, rec=e.record_get(), mission=e.mission_get(), snapshot=snapshot(e), groups=e.get_groups(),
               len_hist=np.array(len_hist) if len(len_hist) == K else None, finished=e.get_finished(), legs=legs)
    if score:
        run["score"], run["mission_scores"] = e.score_get(), e.mission_scores()
        if more:   # a scored engine that stops scoring goes on as one that never scored
            e.score_stop()
    if more:
        e.sim_steps(more, 2, 5e-3)
        run["snapshot_more"] = snapshot(e)
    e.close()
    _RUNS[key] = run
    return run


def base_run(lib, sh, **cfg):
    return mission_run(lib, sh, block=1, **cfg)


# ------------------------------------------------------------------ 1. mission sweep equals the recorder
def case_sweep_equals_recorder(lib, sh, **cfg):
    run = base_run(lib, sh, **cfg)
    ms, sc = run["mission"], run["score"]
    print(f"legs consumed {np.bincount(ms['leg'], minlength=L + 1).tolist()}, finished {int(run['finished'].sum())} of {sh.B}, "
          f"flights {np.bincount(sc['flights'], minlength=5).tolist()}, longest flight {int((sc['steps'] + sc['tail_steps']).max())} periods, "
          f"last leg consumed in period (10 / 50 / 90 %) {np.percentile(ms['leg_period'][:, L - 1], [10, 50, 90]).tolist()}")
    holds = (ms["leg"] == L) & (run["finished"] != 0)
    assert holds.any() and (run["finished"] == 0).any()           # some have consumed all legs and hold, others are in mid-flight
    assert (sc["overflow"] == 0).all() and sc["flights"].max() == 4 and (sc["steps"] + sc["tail_steps"]).max() <= 1500
    done = ms["leg_code"] == REPLAN_DONE
    assert (done & (run["legs"]["kind"] == LEG_CIRCLE)).any() and (done & (run["legs"]["kind"] == LEG_WAYPOINTS)).any()
    assert (sc["tail_steps"][holds] > 0).any()                    # tail_rows = 0: the periods a quadrotor holds its last row
    assert (sc["fallbacks"] <= sc["steps"] + sc["tail_steps"]).all()
    assert_table(run, run["len_hist"], "sim_steps")


def case_sweep_step_path(lib, sh, **cfg):
    run = mission_run(lib, sh, path="step", **cfg)
    assert (run["mission"]["installed"] >= 1).all() and (run["score"]["overflow"] == 0).all()
    assert_table(run, run["len_hist"], "step")


# ------------------------------------------------------------------ 2. tail
def case_tail(lib, sh):
    base, run = base_run(lib, sh), mission_run(lib, sh, tail_rows=50)
    assert_table(run, base["len_hist"], "tail_rows = 50")
    a, b = base["score"], run["score"]
    for k in (9, 10, 11, 12, 13, 14, 15):                         # what every period updates does not know about the tail
        assert np.array_equal(a[SCORE_FIELDS[k]], b[SCORE_FIELDS[k]]), SCORE_FIELDS[k]
    assert np.array_equal(a["flights"], b["flights"]) and np.array_equal(a["steps"] + a["tail_steps"], b["steps"] + b["tail_steps"])
    moved = a["steps"] - b["steps"]
    assert (moved >= 0).all() and (moved <= 50).all() and (moved > 0).any()   # at most the last 50 rows of a flight move to the tail


# ------------------------------------------------------------------ 3. overflow
def case_overflow(lib, sh):
    base, run = base_run(lib, sh), mission_run(lib, sh, F=2)
    assert_table(run, base["len_hist"], "flights = 2")
    a, b = base["score"], run["score"]
    for name in SCORE_FIELDS + SCORE_DERIVED:
        assert np.array_equal(a[name][:, :2], b[name], equal_nan=True), name
    later = (a["steps"] + a["tail_steps"])[:, 2:].sum(axis=1)
    assert np.array_equal(b["overflow"], later) and (later > 0).any()
    assert np.array_equal(b["flights"], np.minimum(a["flights"], 2))
    assert_same(base["snapshot"], run["snapshot"])                # and the neighbours of the table are what they were


# ------------------------------------------------------------------ 4. host replans, no mission
def case_host_replans(lib, sh, F=4):
    B, R = sh.B, sh.R
    x0, traj, lens, _, wp = sweep(sh, seed=73)
    e = start_engine(lib, B, x0, traj, lens)
    K = 6 * R
    e.score_start(F, 0)
    e.record_start(fields=REC_FIELDS, every=1, capacity=K)
    len_hist, opened = [], np.ones(B, np.int64)
    for j in range(6):
        len_hist += [lengths(e)] * R
        e.sim_steps(R, 2, 5e-3)
        assert (e.score_get()["flights"] == np.minimum(opened, F)).all()    # slots open as flights are installed: with their first period
        codes = e.replan(wp[:, j % L], sh.speeds[1], sh.speeds[1], DT)      # mask None: whoever has finished
        opened += codes == REPLAN_DONE
    run = dict(K=K, F=F, tail_rows=0, rec=e.record_get(), score=e.score_get())
    e.close()
    print(f"host replans: flights {np.bincount(run['score']['flights'], minlength=F + 1).tolist()}, overflow {run['score']['overflow'].tolist()[:8]}")
    assert run["score"]["flights"].max() >= 3
    assert_table(run, np.array(len_hist), "host replans")


# ------------------------------------------------------------------ 5. scoring changes nothing
def case_changes_nothing(lib, sh, gsh):
    more = 7
    scored, plain = mission_run(lib, sh, more=more), mission_run(lib, sh, more=more, score=False)
    assert_same(plain["snapshot"], scored["snapshot"])
    assert_same(plain["rec"], scored["rec"], REC_KEYS)
    assert_same(plain["mission"], scored["mission"], ("leg", "installed", "leg_code", "leg_period"))
    assert_same(plain["snapshot_more"], scored["snapshot_more"])  # behind score_stop
    # blocks of one period and blocks of sh.block periods, one group and two (a group holds at least 8 quadrotors): the same table
    one, split = mission_run(lib, gsh), mission_run(lib, gsh, tune=dict(groups=2))
    assert scored["groups"] == 1 and one["groups"] == 1 and split["groups"] == 2
    assert (split["score"]["flights"] >= 2).all()
    for a, b in ((base_run(lib, sh), scored), (one, split)):
        for name in SCORE_FIELDS + SCORE_DERIVED + ("flights", "overflow"):
            assert np.array_equal(a["score"][name], b["score"][name], equal_nan=True), name
    assert_same(one["snapshot"], split["snapshot"])


# ------------------------------------------------------------------ 6. mission_scores
def case_mission_scores(lib, sh):
    run = base_run(lib, sh)
    ms, sc, got = run["mission"], run["score"], run["mission_scores"]
    assert ms["leg_code"][0, 1] == REPLAN_TOO_LONG and ms["leg"][0] >= 2
    assert set(got) == set(SCORE_FIELDS + SCORE_DERIVED)
    hits = 0
    for b in range(sh.B):
        for l in range(L):
            slot = None
            if ms["leg_code"][b, l] == REPLAN_DONE:
                match = [f for f in range(sc["flights"][b]) if sc["first_period"][b, f] == ms["leg_period"][b, l] + 1]
                assert len(match) <= 1
                slot = match[0] if match else None
            for name in got:
                v = got[name][b, l]
                assert got[name].shape == (sh.B, L)
                if slot is None:
                    assert v == -1 if got[name].dtype == np.int64 else np.isnan(v), (name, b, l)
                else:
                    assert np.array_equal(v, sc[name][b, slot], equal_nan=True), (name, b, l)
            hits += slot is not None
    assert hits >= sh.B and got["steps"][0, 1] == -1 and np.isnan(got["peak_speed"][0, 1])
    flown = got["steps"] > 0                                      # the sweep: faster legs reach higher speeds
    assert (got["peak_speed"][flown] > 0).all()
    # a period between mission_set and score_start: the two do not count the same periods
    x0, traj, lens, legs, wp = sweep(sh)
    e = start_engine(lib, sh.B, x0, traj, lens)
    with pytest.raises(ValueError):
        e.mission_scores()                                        # nothing running
    e.mission_set_legs(legs, wp, dt=DT)
    e.sim_steps(1, 2, 5e-3)
    e.score_start(2)
    e.sim_steps(2, 2, 5e-3)
    with pytest.raises(ValueError):
        e.mission_scores()
    e.mission_set_legs(legs, wp, dt=DT)
    e.score_clear()
    e.sim_steps(2, 2, 5e-3)
    assert e.mission_scores()["steps"].shape == (sh.B, L)
    e.close()


# ------------------------------------------------------------------ 7. rules
def case_rules(lib, B=8):
    from test_circle_mission import config
    x0, traj, lens = hover_slots(B, 60, 75)
    e = Engine(config(B), lib_path=lib)
    assert b"mpcq 0.6.7" in e.lib.mpcq_version()
    expect_rc(MPCQ_ERR_STATE, e.score_start, 2)                   # before set_trajectories
    e.set_trajectories(traj, lens)
    e.sim_reset(x0)
    for fn in (e.lib.mpcq_score_clear, e.lib.mpcq_score_stop):
        assert fn(e.h) == MPCQ_ERR_STATE
    assert e.lib.mpcq_score_get(e.h, None, None, None, None) == MPCQ_ERR_STATE
    for F, tail in ((0, 0), (-1, 0), (2, -1), (2 ** 31 // (16 * B) + 1, 0)):   # the last: B x F x 16 >= 2^31, refused before any allocation
        expect_rc(MPCQ_ERR_INVALID, e.score_start, F, tail)
    assert e.lib.mpcq_score_stop(e.h) == MPCQ_ERR_STATE           # none of the refused calls started a score
    e.score_start(2, 0)
    assert e.lib.mpcq_score_get(e.h, None, None, None, None) == 0  # every pointer may be NULL
    sc = e.score_get()
    assert sc["periods"] == 0 and (sc["flights"] == 0).all() and (sc["first_period"] == -1).all() and (sc["last_period"] == -1).all()
    assert all((sc[n] == 0).all() for n in SCORE_FIELDS if n not in ("first_period", "last_period")) and np.isnan(sc["rmse_pos"]).all()
    expect_rc(MPCQ_ERR_STATE, e.sim_run, 2, 2, 5e-3)              # one persistent launch: refused while a score is running
    e.solve(x0)                                                   # not a period
    assert e.score_get()["periods"] == 0
    e.sim_steps(3, 2, 5e-3)
    sc = e.score_get()
    assert sc["periods"] == 3 and (sc["flights"] == 1).all() and (sc["first_period"][:, 0] == 0).all() and (sc["last_period"][:, 0] == 2).all()
    assert (sc["steps"][:, 0] + sc["tail_steps"][:, 0] == 3).all() and (sc["steps"][:, 0] == 2).all() and (sc["rows"][:, 0] == 2).all()
    assert (sc["finished"][:, 0] == 1).all() and (sc["first_period"][:, 1] == -1).all()
    e.score_start(3, 0)                                           # twice: replaces and resets
    sc = e.score_get()
    assert sc["steps"].shape == (B, 3) and sc["periods"] == 0 and (sc["flights"] == 0).all() and (sc["steps"] == 0).all()
    e.sim_steps(2, 2, 5e-3)                                       # started in mid-flight (here: holding): the partial flight is slot 0
    sc = e.score_get()
    assert (sc["flights"] == 1).all() and (sc["tail_steps"][:, 0] == 2).all() and (sc["steps"] == 0).all()
    e.score_clear()                                               # zeroes and keeps scoring
    sc = e.score_get()
    assert sc["periods"] == 0 and (sc["flights"] == 0).all() and (sc["tail_steps"] == 0).all() and (sc["last_period"] == -1).all()
    e.step(x0)
    sc = e.score_get()
    assert sc["periods"] == 1 and (sc["tail_steps"][:, 0] == 1).all() and (sc["first_period"][:, 0] == 0).all()
    e.reset()                                                     # allowed while a score is running
    e.set_trajectories(traj, lens)                                # cursor 0: the next period opens slot 1
    e.sim_steps(1, 2, 5e-3)
    sc = e.score_get()
    assert (sc["flights"] == 2).all() and (sc["steps"][:, 1] == 1).all() and (sc["first_period"][:, 1] == 1).all()
    e.score_stop()
    expect_rc(MPCQ_ERR_STATE, e.score_stop)
    e.sim_run(2, 2, 5e-3)                                         # legal again
    e.close()


# ------------------------------------------------------------------ lane emulator (CPU)
def test_emu_sweep_equals_recorder(emu):
    case_sweep_equals_recorder(emu, EMU_SHAPE)


def test_emu_sweep_step_path(emu):
    case_sweep_step_path(emu, EMU_SHAPE)


def test_emu_tail(emu):
    case_tail(emu, EMU_SHAPE)


def test_emu_overflow(emu):
    case_overflow(emu, EMU_SHAPE)


def test_emu_host_replans(emu):
    case_host_replans(emu, EMU_SHAPE)


def test_emu_scoring_changes_nothing(emu):
    case_changes_nothing(emu, EMU_SHAPE, EMU_GROUPS_SHAPE)


def test_emu_mission_scores(emu):
    case_mission_scores(emu, EMU_SHAPE)


def test_emu_rules(emu):
    case_rules(emu)


# ------------------------------------------------------------------ MI355X
gpu = pytest.mark.gpu


@gpu
@pytest.mark.parametrize("precision", [0, 1])
def test_gpu_sweep_equals_recorder(precision):
    case_sweep_equals_recorder(None, GPU_SHAPE, precision=precision)


@gpu
@pytest.mark.parametrize("precision", [0, 1])
def test_gpu_sweep_step_path(precision):
    case_sweep_step_path(None, GPU_SHAPE, precision=precision)


@gpu
def test_gpu_tail():
    case_tail(None, GPU_SHAPE)


@gpu
def test_gpu_overflow():
    case_overflow(None, GPU_SHAPE)


@gpu
def test_gpu_host_replans():
    case_host_replans(None, GPU_SHAPE)


@gpu
def test_gpu_scoring_changes_nothing():
    case_changes_nothing(None, GPU_SHAPE, GPU_SHAPE)


@gpu
def test_gpu_mission_scores():
    case_mission_scores(None, GPU_SHAPE)


@gpu
def test_gpu_rules():
    case_rules(None, B=256)

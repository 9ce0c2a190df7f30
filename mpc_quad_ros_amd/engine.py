"""Batched engine handle over the C ABI (include/mpcq.h): B quadrotors advanced in lockstep on
one MI355X, all state resident in HBM.  Thin: every method is one C call plus numpy marshalling."""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib
from .params import NU, NX, NY, EngineConfig


# decimal fields of mpcq_get_qp_iter (include/mpcq.h)
def qp_passes(it):
    """Riccati factorisations of the solve (active-set passes + interior-point iterations)."""
    return np.asarray(it) % 1000


def qp_fallback(it):
    """True where the warm active-set attempt was given up or skipped and the solve went through the interior point."""
    return (np.asarray(it) // 1000) % 10 != 0


def qp_flip(it):
    """True where the solve carries the flip mark (the next one skips the warm attempt)."""
    return (np.asarray(it) // 10000) % 10 != 0


def qp_warm_exit(it):
    """MPCQ_WARM_* code: why the warm attempt ended without a solution (0: it succeeded / there was none)."""
    return np.asarray(it) // 100000


def order_bin(it):
    """Cost bin of mpcq::order_kernel (0 = predicted most expensive) for a qp_iter value of the previous period."""
    it = np.maximum(np.asarray(it), 0)      # (a negative value is not one the solver writes: binned like a cold start, as on the device)
    total = it % 1000
    cost = np.where(it == 0, 15, np.minimum(total, 15))
    cost = np.where(((it // 1000) % 100 != 0) & (cost < 8), 8, cost)
    return 15 - cost


WARM_BUDGET, WARM_PINS, WARM_WRONG, WARM_BOUNCE, WARM_NUMERIC, WARM_SKIPPED = 1, 2, 3, 4, 5, 6
SOLVE_LOW_ACCURACY = 8
# per-quadrotor result codes of Engine.replan (include/mpcq.h MPCQ_REPLAN_*)
REPLAN_DONE, REPLAN_SKIPPED, REPLAN_BAD_INPUT, REPLAN_SINGULAR, REPLAN_LIMITS, REPLAN_TOO_LONG = 0, 1, -1, -2, -3, -4
# circle flights of Engine.replan_circle (include/mpcq.h MPCQ_CIRCLE_*) and leg kinds of Engine.mission_set_legs (MPCQ_LEG_*)
CIRCLE_KINDS = {"acc_dec": 0, "constant": 1, "accelerating": 2}
LEG_WAYPOINTS, LEG_CIRCLE = 0, 1
LEG_DTYPE = np.dtype([("kind", np.int32), ("reserved", np.int32), ("v_max", np.float64), ("a_max", np.float64), ("radius", np.float64)])


# flight recorder fields (include/mpcq.h MPCQ_RECORD_*): name -> bit
RECORD_FIELDS = {"x_odom": 1, "x_ref": 2, "w_odom": 4, "x_pred_odom": 8, "cost_solution": 16, "drag": 32, "rgp_mu": 64, "rgp_C": 128,
                 "solver": 256}
RECORD_DEFAULT = ("x_odom", "x_ref", "w_odom", "x_pred_odom", "cost_solution", "drag", "rgp_mu", "solver")
# flight scoreboard (include/mpcq.h, mpcq_score_*): the fields of a row in order, and what score_get derives from them
SCORE_FIELDS = ("steps", "sum_epos2", "sum_evel2", "max_epos2", "sum_rms_pos", "max_v2", "max_vref2", "sum_cost", "tail_steps", "bad_status",
                "fallbacks", "factorisations", "first_period", "last_period", "rows", "finished")
SCORE_INT = (0, 8, 9, 10, 11, 12, 13, 14, 15)
SCORE_DERIVED = ("rmse_pos", "mean_rms_pos", "peak_speed")


def score_fields(table):
    """A score table [..., 16] as a dict of its fields by name (counts and period numbers int64) plus the derived fields."""
    out = {name: table[..., k].astype(np.int64) if k in SCORE_INT else table[..., k].copy() for k, name in enumerate(SCORE_FIELDS)}
    with np.errstate(divide="ignore", invalid="ignore"):
        n = np.where(out["steps"] > 0, out["steps"], np.nan)
        out["rmse_pos"] = np.sqrt(out["sum_epos2"] / n)
        out["mean_rms_pos"] = out["sum_rms_pos"] / n
        out["peak_speed"] = np.where(out["steps"] > 0, np.sqrt(out["max_v2"]), np.nan)
    return out


class Engine:
    def __init__(self, cfg: EngineConfig, lib_path: str | None = None):
        self.cfg = cfg
        self.lib = _lib.load(lib_path)
        self._c = cfg.to_c()
        h = ctypes.c_void_p()
        self._check(self.lib.mpcq_create_sized(ctypes.byref(self._c), ctypes.sizeof(self._c), ctypes.byref(h)))
        self.h = h
        self.B, self.N, self.nb = cfg.batch, cfg.N, cfg.nb
        self._periods = 0   # periods issued through this handle (what the recorder, a mission and the scoreboard count)

    def _check(self, rc):
        if rc != 0:
            raise _lib.MpcqError(f"mpcq error {rc}: {self.lib.mpcq_last_error().decode()}")

    def close(self):
        if getattr(self, "h", None):
            self.lib.mpcq_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @staticmethod
    def _f(a, shape=None):
        if a is None:
            return None
        a = np.ascontiguousarray(a, dtype=np.float64)
        return a if shape is None else a.reshape(shape)

    # ---- state
    def reset(self):
        self._check(self.lib.mpcq_reset(self.h))

    def set_trajectories(self, traj, lengths=None):
        traj = self._f(traj)
        if traj.ndim != 3 or traj.shape[0] != self.B or traj.shape[2] != NX:
            raise ValueError(f"traj must be [B={self.B}, T, 13]")
        if lengths is None:
            lengths = np.full(self.B, traj.shape[1])
        lengths = np.ascontiguousarray(lengths, dtype=np.int32)
        self._check(self.lib.mpcq_set_trajectories(self.h, _lib.d(traj), _lib.i(lengths), traj.shape[1]))
        self._tmax = traj.shape[1]

    # ---- continuous operation: replace the flights of some quadrotors while the others keep flying
    def replan(self, wp, v_max, a_max, dt=0.01, derivative_to_optimize=4, start=None, mask=None):
        """Minimum-snap flights planned on the device from start [B,3] (None: the on-device plant's position) through wp [B,n_wp,3]
        for the selected quadrotors (mask [B] != 0; None: those whose finished flag is set), installed in their slots with the
        cursor at 0.  Returns the per-quadrotor codes [B] (REPLAN_*)."""
        wp = self._f(wp)
        if wp.ndim != 3 or wp.shape[0] != self.B or wp.shape[2] != 3:
            raise ValueError(f"wp must be [B={self.B}, n_wp, 3]")
        start = self._f(start, (self.B, 3))
        mask = None if mask is None else np.ascontiguousarray(mask, dtype=np.int32).reshape(self.B)
        out = np.zeros(self.B, np.int32)
        self._check(self.lib.mpcq_replan(self.h, _lib.d(start), _lib.d(wp), wp.shape[1], float(v_max), float(a_max),
                                         int(derivative_to_optimize), float(dt), _lib.i(mask), _lib.i(out)))
        return out

    def replan_nonlinear(self, wp, v_max, a_max, dt=0.01, derivative_to_optimize=3, start=None, mask=None, opts=None, return_pieces=False):
        """replan with the reference generator's nonlinear stage (mpcq_replan_nonlinear): segment times and free vertex derivatives
        optimised by Subplex under soft speed / acceleration limits, exactly the host library's mpcq_minsnap_nonlinear.  opts: dict of
        overrides of the defaults (_lib.nl_defaults()).  Returns (codes [B], info [B,6]: f start, f end, evaluations, duration, peak
        speed, peak acceleration -- NaN rows where no flight was made); with return_pieces also pieces [B,n_wp,33] and
        d_free [B,n_wp-1,3,3]."""
        wp = self._f(wp)
        if wp.ndim != 3 or wp.shape[0] != self.B or wp.shape[2] != 3:
            raise ValueError(f"wp must be [B={self.B}, n_wp, 3]")
        start = self._f(start, (self.B, 3))
        mask = None if mask is None else np.ascontiguousarray(mask, dtype=np.int32).reshape(self.B)
        o = _lib.nl_options(opts)
        out, info = np.zeros(self.B, np.int32), np.zeros((self.B, 6))
        n_wp = wp.shape[1]
        pieces = np.zeros((self.B, n_wp, 33)) if return_pieces else None
        d_free = np.zeros((self.B, max(n_wp - 1, 0), 3, 3)) if return_pieces else None
        self._check(self.lib.mpcq_replan_nonlinear(self.h, _lib.d(start), _lib.d(wp), n_wp, float(v_max), float(a_max),
                                                   int(derivative_to_optimize), float(dt), _lib.i(mask), _lib.i(out),
                                                   None if o is None else ctypes.byref(o), _lib.d(info), _lib.d(pieces), _lib.d(d_free)))
        return (out, info, pieces, d_free) if return_pieces else (out, info)

    def replan_circle(self, radius, v_max, kind="acc_dec", dt=0.01, t_max=10.0, start=None, mask=None):
        """Circle flights generated on the device (mpcq_replan_circle) -- what trajectories.circle_trajectory(kind, radius[b], v_max[b], dt,
        t_max, start_b) makes on the host -- for the selected quadrotors, installed as replan installs.  radius, v_max: scalars or [B];
        kind: 'acc_dec' (the reference node's circle request), 'constant' or 'accelerating' (the only one that reads t_max); start
        [B,3] (None: the on-device plant's position).  Returns the per-quadrotor codes [B] (REPLAN_*)."""
        if kind not in CIRCLE_KINDS:
            raise ValueError(f"kind must be one of {sorted(CIRCLE_KINDS)}")
        radius = np.ascontiguousarray(np.broadcast_to(np.asarray(radius, dtype=np.float64), (self.B,)))
        v_max = np.ascontiguousarray(np.broadcast_to(np.asarray(v_max, dtype=np.float64), (self.B,)))
        start = self._f(start, (self.B, 3))
        mask = None if mask is None else np.ascontiguousarray(mask, dtype=np.int32).reshape(self.B)
        out = np.zeros(self.B, np.int32)
        self._check(self.lib.mpcq_replan_circle(self.h, _lib.d(start), _lib.d(radius), _lib.d(v_max), CIRCLE_KINDS[kind], float(dt), float(t_max),
                                                _lib.i(mask), _lib.i(out)))
        return out

    def replace_trajectories(self, idx, traj, lengths):
        """Host-made rows traj [count, Tmax, 13] (the first lengths[j] used) into the slots of quadrotors idx [count]."""
        idx = np.ascontiguousarray(idx, dtype=np.int32).reshape(-1)
        traj = self._f(traj)
        lengths = np.ascontiguousarray(lengths, dtype=np.int32).reshape(-1)
        tmax = getattr(self, "_tmax", None)
        if tmax is None or traj.shape != (len(idx), tmax, NX) or lengths.shape != idx.shape:
            raise ValueError(f"traj must be [count={len(idx)}, Tmax={tmax}, 13] and lengths [count]")
        self._check(self.lib.mpcq_replace_trajectories(self.h, _lib.i(idx), len(idx), _lib.d(traj), _lib.i(lengths)))

    def get_trajectories(self):
        """(traj [B, Tmax, 13], lengths [B]) as they are on the device now."""
        tmax = getattr(self, "_tmax", None)
        if tmax is None:
            raise _lib.MpcqError("get_trajectories needs set_trajectories first")
        traj, lengths = np.zeros((self.B, tmax, NX)), np.zeros(self.B, np.int32)
        self._check(self.lib.mpcq_get_trajectories(self.h, _lib.d(traj), _lib.i(lengths)))
        return traj, lengths

    # ---- device missions: a queue of upcoming flights per quadrotor, the next one installed on the device in the period a flight ends
    def mission_set(self, wp, v_max, a_max, order=4, dt=0.01, nonlinear=False, opts=None, leg0=None):
        """Queue wp [B, L, n_wp, 3]: behind every period (sim_steps, sim_control_periods, step, step_device_async) a quadrotor whose
        finished flag is set and that has a leg left gets the flight replan (nonlinear: replan_nonlinear with `opts`) would plan from
        where it stands through wp[b, leg[b]], without a host round trip.  leg0 [B]: the leg counters to start from (a checkpoint's
        mission_get()["leg"]; None: 0).  Calling it again replaces the queue and resets the log."""
        wp = self._f(wp)
        if wp.ndim != 4 or wp.shape[0] != self.B or wp.shape[3] != 3:
            raise ValueError(f"wp must be [B={self.B}, L, n_wp, 3]")
        leg0 = None if leg0 is None else np.ascontiguousarray(leg0, dtype=np.int32).reshape(self.B)
        o = _lib.nl_options(opts) if nonlinear else None
        self._check(self.lib.mpcq_mission_set(self.h, _lib.d(wp), wp.shape[1], wp.shape[2], float(v_max), float(a_max), int(order), float(dt),
                                              int(bool(nonlinear)), None if o is None else ctypes.byref(o), _lib.i(leg0)))
        self._mission_legs = wp.shape[1]
        self._mission_t0 = self._periods

    def mission_set_legs(self, legs, wp=None, order=4, dt=0.01, nonlinear=False, opts=None, leg0=None):
        """mission_set with a kind and limits per leg (mpcq_mission_set_legs).  legs: a structured array [B, L] of LEG_DTYPE, or a dict
        of [B, L] arrays (or scalars) `kind` (LEG_WAYPOINTS / LEG_CIRCLE, or 'waypoints' / 'circle'), `v_max`, `a_max` and -- for circle
        legs -- `radius` (trajectories.mission_legs builds one).  A waypoint leg is replan's flight through wp[b, leg] with the leg's
        limits, a circle leg replan_circle's 'acc_dec' circle of the leg's radius and v_max from where the quadrotor stands.
        wp [B, L, n_wp, 3]; None if every leg is a circle."""
        if isinstance(legs, dict):
            unknown = set(legs) - {"kind", "v_max", "a_max", "radius"}
            if unknown or not {"kind", "v_max", "a_max"} <= set(legs):
                raise ValueError("legs needs kind, v_max, a_max and (circle legs) radius")
            shape = np.broadcast_shapes(*(np.shape(v) for v in legs.values()))
            if len(shape) != 2 or shape[0] != self.B:
                raise ValueError(f"the arrays of legs must be [B={self.B}, L]")
            from .trajectories import mission_legs
            legs = mission_legs(self.B, shape[1], legs["v_max"], legs["a_max"], legs["kind"], legs.get("radius", 0.0))
        legs = np.ascontiguousarray(legs)
        if legs.dtype != LEG_DTYPE or legs.ndim != 2 or legs.shape[0] != self.B:
            raise ValueError(f"legs must be a [B={self.B}, L] array of engine.LEG_DTYPE")
        L, n_wp = legs.shape[1], 0
        if wp is not None:
            wp = self._f(wp)
            if wp.ndim != 4 or wp.shape[0] != self.B or wp.shape[1] != L or wp.shape[3] != 3:
                raise ValueError(f"wp must be [B={self.B}, L={L}, n_wp, 3]")
            n_wp = wp.shape[2]
        leg0 = None if leg0 is None else np.ascontiguousarray(leg0, dtype=np.int32).reshape(self.B)
        o = _lib.nl_options(opts) if nonlinear else None
        self._check(self.lib.mpcq_mission_set_legs(self.h, legs.ctypes.data_as(ctypes.POINTER(_lib.Leg)), _lib.d(wp), L, n_wp, int(order), float(dt),
                                                   int(bool(nonlinear)), None if o is None else ctypes.byref(o), _lib.i(leg0)))
        self._mission_legs = L
        self._mission_t0 = self._periods

    def mission_get(self):
        """The mission's state: leg [B] (legs consumed), installed [B] (flights installed), last_code [B], leg_code [B, L] (REPLAN_*;
        REPLAN_SKIPPED: not consumed), leg_period [B, L] (period number since mission_set in which the leg was consumed, -1: not yet),
        info [B, 6] (nonlinear: replan_nonlinear's info of the last installed flight; else NaN)."""
        L = getattr(self, "_mission_legs", None)
        if L is None:
            raise _lib.MpcqError("mission_get needs mission_set first")
        B = self.B
        out = dict(leg=np.zeros(B, np.int32), installed=np.zeros(B, np.int32), last_code=np.zeros(B, np.int32),
                   leg_code=np.zeros((B, L), np.int32), leg_period=np.zeros((B, L), np.int32), info=np.zeros((B, 6)))
        self._check(self.lib.mpcq_mission_get(self.h, _lib.i(out["leg"]), _lib.i(out["installed"]), _lib.i(out["last_code"]),
                                              _lib.i(out["leg_code"]), _lib.i(out["leg_period"]), _lib.d(out["info"])))
        return out

    def mission_stop(self):
        self._check(self.lib.mpcq_mission_stop(self.h))
        self._mission_legs = None

    # ---- flight recorder: per-period rows of selected quadrotors written on the device, read once
    def record_start(self, quads=None, fields=RECORD_DEFAULT, every=1, capacity=1000):
        """Record quadrotors `quads` (None: all, else indices in the order record_get returns them) from the next period on: the fields
        named (RECORD_FIELDS; the default drops the RGP fields on an engine without RGP), every `every`-th period, up to `capacity`
        rows per quadrotor (later periods are counted as dropped)."""
        if fields is RECORD_DEFAULT and not self.nb:
            fields = tuple(f for f in fields if not f.startswith("rgp"))
        unknown = set(fields) - set(RECORD_FIELDS)
        if unknown:
            raise ValueError(f"unknown record fields {sorted(unknown)}")
        mask = 0
        for f in fields:
            mask |= RECORD_FIELDS[f]
        q = None if quads is None else np.ascontiguousarray(quads, dtype=np.int32).reshape(-1)
        self._check(self.lib.mpcq_record_start(self.h, _lib.i(q), 0 if q is None else len(q), mask, int(every), int(capacity)))
        self._rec = dict(quads=np.arange(self.B, dtype=np.int32) if q is None else q.copy(), fields=mask)

    def record_info(self):
        """(rows, dropped, periods): rows recorded, periods dropped because the buffer was full, periods counted since record_start."""
        rows, dropped, periods = ctypes.c_int32(), ctypes.c_int64(), ctypes.c_int64()
        self._check(self.lib.mpcq_record_info(self.h, ctypes.byref(rows), ctypes.byref(dropped), ctypes.byref(periods)))
        return rows.value, dropped.value, periods.value

    def record_get(self):
        """The recording so far, keyed by the reference's log names: x_odom, x_ref, x_pred_odom [count,T,13], w_odom [count,T,4],
        cost_solution [count,T], v_body, a_drag [count,T,3], rgp_mu_g_t [count,T,3,nb], rgp_C_g_t [count,T,3,nb,nb], status, qp_iter,
        idx (the cursor the step used), finished [count,T] -- the fields recorded -- and period [T], quads [count], dropped."""
        rows, dropped, _ = self.record_info()
        rec = getattr(self, "_rec", None)
        quads, mask = rec["quads"], rec["fields"]
        n, nb = len(quads), self.nb
        out = dict(period=np.zeros(rows, np.int64), quads=quads.copy(), dropped=dropped)
        self._check(self.lib.mpcq_record_get_periods(self.h, _lib.l(out["period"])))

        def get(bit, width):
            a = np.zeros((n, rows, width))
            self._check(self.lib.mpcq_record_get(self.h, bit, _lib.d(a)))
            return a
        for name, bit, shape in (("x_odom", 1, (NX,)), ("x_ref", 2, (NX,)), ("w_odom", 4, (NU,)), ("x_pred_odom", 8, (NX,)),
                                 ("cost_solution", 16, ()), ("rgp_mu_g_t", 64, (3, nb)), ("rgp_C_g_t", 128, (3, nb, nb))):
            if mask & bit:
                out[name] = get(bit, int(np.prod(shape, dtype=np.int64))).reshape((n, rows) + shape)
        if mask & 32:
            d = get(32, 6)
            out["v_body"], out["a_drag"] = d[:, :, 0:3].copy(), d[:, :, 3:6].copy()
        if mask & 256:
            sv = np.zeros((n, rows, 4), np.int32)
            self._check(self.lib.mpcq_record_get_solver(self.h, _lib.i(sv)))
            for k, name in enumerate(("status", "qp_iter", "idx", "finished")):
                out[name] = sv[:, :, k].copy()
        return out

    def record_clear(self):
        """Empty the buffers (rows and dropped to 0); selection, fields and the period count stay."""
        self._check(self.lib.mpcq_record_clear(self.h))

    def record_stop(self):
        self._check(self.lib.mpcq_record_stop(self.h))
        self._rec = None

    # ---- incident recorder: a ring of the recorder's rows per watched quadrotor, stopped on the device by a rule of its own
    def blackbox_start(self, rules, quads=None, fields=RECORD_DEFAULT, pre=50, post=20):
        """Watch quadrotors `quads` (None: all, else indices in the order the read-outs return them) from the next period on: each keeps
        the last pre + 1 + post rows of the fields named (RECORD_FIELDS, as record_start takes them) in a ring on the device, and the ring
        stops `post` periods after the quadrotor's rule first fires.  rules: [count] of params.BLACKBOX_RULE_DTYPE in the order of
        `quads` (params.blackbox_rules builds them)."""
        from .params import BLACKBOX_RULE_DTYPE
        if fields is RECORD_DEFAULT and not self.nb:
            fields = tuple(f for f in fields if not f.startswith("rgp"))
        unknown = set(fields) - set(RECORD_FIELDS)
        if unknown:
            raise ValueError(f"unknown record fields {sorted(unknown)}")
        mask = 0
        for f in fields:
            mask |= RECORD_FIELDS[f]
        q = None if quads is None else np.ascontiguousarray(quads, dtype=np.int32).reshape(-1)
        count = self.B if q is None else len(q)
        rules = np.ascontiguousarray(rules)
        if rules.dtype != BLACKBOX_RULE_DTYPE or rules.shape != (count,):
            raise ValueError(f"rules must be a [count={count}] array of params.BLACKBOX_RULE_DTYPE")
        self._check(self.lib.mpcq_blackbox_start(self.h, _lib.i(q), 0 if q is None else len(q), mask, int(pre), int(post), rules.ctypes.data))
        self._bb = dict(quads=np.arange(self.B, dtype=np.int32) if q is None else q.copy(), fields=mask, D=int(pre) + 1 + int(post))

    def _bb_state(self):
        bb = getattr(self, "_bb", None)
        if bb is None:
            raise _lib.MpcqError("no black box running (blackbox_start first)")
        return bb

    def blackbox_info(self):
        """The state of every watched quadrotor, in the order of blackbox_start: fired_period [count] (-1: not fired), cause (BB_* bits
        of the firing period), state (0 armed, 1 fired, 2 frozen), rows (valid rows of the ring), fired_row (index of the firing row in the
        read-out, -1), and periods (counted since blackbox_start), quads."""
        bb = self._bb_state()
        n = len(bb["quads"])
        out = dict(fired_period=np.zeros(n, np.int64), cause=np.zeros(n, np.int32), state=np.zeros(n, np.int32), rows=np.zeros(n, np.int32),
                   fired_row=np.zeros(n, np.int32))
        periods = ctypes.c_int64()
        self._check(self.lib.mpcq_blackbox_info(self.h, _lib.l(out["fired_period"]), _lib.i(out["cause"]), _lib.i(out["state"]), _lib.i(out["rows"]),
                                                _lib.i(out["fired_row"]), ctypes.byref(periods)))
        out["periods"], out["quads"] = periods.value, bb["quads"].copy()
        return out

    def blackbox_get(self, which=None):
        """The rings of a subset of the watched quadrotors, gathered on the device in time order and left-aligned: which = None (all),
        "fired" (those whose rule has fired) or positions in the selection of blackbox_start.  Keys as record_get's with shape
        [n, D, ...] (rows beyond rows[i] NaN, -1 for status, qp_iter, idx, finished), period [n, D] (-1 beyond rows), and rows,
        fired_row, fired_period, cause, state, quads [n], which [n] (the positions read)."""
        bb = self._bb_state()
        info = self.blackbox_info()
        if which is None:
            w = np.arange(len(bb["quads"]), dtype=np.int32)
        elif isinstance(which, str):
            if which != "fired":
                raise ValueError('which must be None, "fired" or positions in the selection')
            w = np.flatnonzero(info["fired_period"] >= 0).astype(np.int32)
        else:
            w = np.ascontiguousarray(which, dtype=np.int32).reshape(-1)
        n, D, nb, mask = len(w), bb["D"], self.nb, bb["fields"]
        out = dict(which=w.copy(), period=np.full((n, D), -1, np.int64))
        self._check(self.lib.mpcq_blackbox_get_periods(self.h, _lib.i(w), n, _lib.l(out["period"])))
        for k in ("rows", "fired_row", "fired_period", "cause", "state", "quads"):
            out[k] = info[k][w].copy()

        def get(bit, width):
            a = np.zeros((n, D, width))
            self._check(self.lib.mpcq_blackbox_get(self.h, bit, _lib.i(w), n, _lib.d(a)))
            return a
        for name, bit, shape in (("x_odom", 1, (NX,)), ("x_ref", 2, (NX,)), ("w_odom", 4, (NU,)), ("x_pred_odom", 8, (NX,)),
                                 ("cost_solution", 16, ()), ("rgp_mu_g_t", 64, (3, nb)), ("rgp_C_g_t", 128, (3, nb, nb))):
            if mask & bit:
                out[name] = get(bit, int(np.prod(shape, dtype=np.int64))).reshape((n, D) + shape)
        if mask & 32:
            d = get(32, 6)
            out["v_body"], out["a_drag"] = d[:, :, 0:3].copy(), d[:, :, 3:6].copy()
        if mask & 256:
            sv = np.zeros((n, D, 4), np.int32)
            self._check(self.lib.mpcq_blackbox_get_solver(self.h, _lib.i(w), n, _lib.i(sv)))
            for k, name in enumerate(("status", "qp_iter", "idx", "finished")):
                out[name] = sv[:, :, k].copy()
        return out

    @staticmethod
    def blackbox_recording(box, j):
        """Item j of a blackbox_get() result as a record_get()-shaped dict of its valid rows (count 1, T = rows[j]): what
        logger.SwarmLogger.from_recording takes, so an incident is written in the reference's pickle layout like any recording."""
        T = int(box["rows"][j])
        meta = ("which", "rows", "fired_row", "fired_period", "cause", "state", "quads", "period")
        out = {k: v[j:j + 1, :T].copy() for k, v in box.items() if k not in meta}
        out["period"], out["quads"], out["dropped"] = box["period"][j, :T].copy(), box["quads"][j:j + 1].copy(), 0
        return out

    def blackbox_rearm(self, mask=None):
        """The selected quadrotors (mask [count] non-zero, in the order of blackbox_start; None: all) back to armed with an empty ring
        that begins with the next period; the others keep what they hold."""
        bb = self._bb_state()
        m = None if mask is None else np.ascontiguousarray(np.asarray(mask) != 0, dtype=np.int32).reshape(len(bb["quads"]))
        self._check(self.lib.mpcq_blackbox_rearm(self.h, _lib.i(m)))

    def blackbox_stop(self):
        self._check(self.lib.mpcq_blackbox_stop(self.h))
        self._bb = None

    # ---- flight scoreboard: every period folded on the device into the row of the flight the quadrotor is flying, read once
    def score_start(self, flights, tail_rows=0):
        """Score every flight from the next period on: `flights` slots per quadrotor, a slot opened by every period whose step used
        cursor 0; the last `tail_rows` rows of a flight (100: the reference's dropped last second) and the periods beyond its end count
        as tail_steps only.  Replaces a running score."""
        self._check(self.lib.mpcq_score_start(self.h, int(flights), int(tail_rows)))
        self._score_flights = int(flights)
        self._score_t0 = self._periods

    def score_get(self):
        """The scoreboard: the sixteen fields of include/mpcq.h by name, each [B, F] (fields 0 and 8..15 int64), flights [B] (slots that
        hold a period), overflow [B] (periods that found no slot), periods, and the derived rmse_pos = sqrt(sum_epos2 / steps),
        mean_rms_pos = sum_rms_pos / steps (the ordinate of the reference's compare_trajectories scatter) and peak_speed = sqrt(max_v2)
        (its abscissa), NaN where steps == 0."""
        F = getattr(self, "_score_flights", None)
        if F is None:
            raise _lib.MpcqError("score_get needs score_start first")
        B = self.B
        t = np.zeros((B, F, len(SCORE_FIELDS)))
        out = dict(flights=np.zeros(B, np.int32), overflow=np.zeros(B, np.int32))
        periods = ctypes.c_int64()
        self._check(self.lib.mpcq_score_get(self.h, _lib.d(t), _lib.i(out["flights"]), _lib.i(out["overflow"]), ctypes.byref(periods)))
        out["periods"] = periods.value
        out.update(score_fields(t))
        return out

    def score_clear(self):
        """Table, slots, overflow and the period count back to their start values; the score stays on."""
        self._check(self.lib.mpcq_score_clear(self.h))
        self._score_t0 = self._periods

    def score_stop(self):
        self._check(self.lib.mpcq_score_stop(self.h))
        self._score_flights = None

    def mission_scores(self):
        """The scoreboard by mission leg: the fields of score_get as [B, L].  Leg l of quadrotor b, installed (leg_code REPLAN_DONE) in
        period p, is the slot whose first_period is p + 1; a leg that was not installed, has not begun or was lost to overflow gives NaN
        (float fields) or -1 (integer fields).  Needs score and mission to count the same periods -- score_start / score_clear and
        mission_set* with no period between them -- else ValueError.  The check rests on this handle's own count of the periods it
        issued (step, step_device_async, sim_steps, sim_control_periods; the library does not report a mission's period count): it does
        not see periods issued on the same engine through the C ABI or another wrapper, nor those of a call that failed part-way; after
        either, start score and mission again before relying on the mapping."""
        if getattr(self, "_score_flights", None) is None or getattr(self, "_mission_legs", None) is None:
            raise ValueError("mission_scores needs a running score and a mission")
        if self._score_t0 != self._mission_t0:   # (periods issued through this handle, counted by step, sim_steps and their like)
            raise ValueError("mission_scores: score and mission do not count the same periods (score_start / score_clear and mission_set* "
                             "with no period between them)")
        sc, ms = self.score_get(), self.mission_get()
        want = np.where(ms["leg_code"] == REPLAN_DONE, ms["leg_period"].astype(np.int64) + 1, -2)            # [B, L]
        first = np.where(sc["steps"] + sc["tail_steps"] > 0, sc["first_period"], -1)                          # [B, F]
        hit = want[:, :, None] == first[:, None, :]                                                           # [B, L, F]
        found, slot = hit.any(axis=2), hit.argmax(axis=2)
        out = {}
        for name in SCORE_FIELDS + SCORE_DERIVED:
            v = np.take_along_axis(sc[name], slot, axis=1)
            out[name] = np.where(found, v, -1 if v.dtype.kind == "i" else np.nan)
        return out

    # ---- the fleet: every quadrotor its own plant (the controller keeps the engine's model)
    def fleet_set(self, plants, period0=0):
        """Fly plants [B] of params.PLANT_DTYPE (params.fleet_defaults / fleet_sample build them) in every plant update from now on:
        sim_steps, sim_control_periods, sim_plant_period.  period0 >= 0 sets the fleet period, which the disturbance windows
        [d_from, d_to) refer to and every plant update advances by one; -1 keeps it.  Calling it again replaces the table."""
        from .params import PLANT_DTYPE
        plants = np.ascontiguousarray(plants)
        if plants.dtype != PLANT_DTYPE or plants.shape != (self.B,):
            raise ValueError(f"plants must be a [B={self.B}] array of params.PLANT_DTYPE")
        self._check(self.lib.mpcq_fleet_set(self.h, plants.ctypes.data_as(ctypes.c_void_p), PLANT_DTYPE.itemsize, int(period0)))

    def fleet_get(self):
        """(plants [B] as they were set, the fleet period)."""
        from .params import PLANT_DTYPE
        plants, period = np.zeros(self.B, PLANT_DTYPE), ctypes.c_int64()
        self._check(self.lib.mpcq_fleet_get(self.h, plants.ctypes.data_as(ctypes.c_void_p), PLANT_DTYPE.itemsize, ctypes.byref(period)))
        return plants, period.value

    def fleet_stop(self):
        """Back to the engine's shared plant."""
        self._check(self.lib.mpcq_fleet_stop(self.h))

    def fleet_drag_truth(self, v):
        """The body-frame drag acceleration [B, 3, M] of every plant of the fleet at body velocities v ([M], [3, M] or [B, 3, M]), from
        the table in numpy (params.fleet_drag_accel): the curve rgp_predict is to be compared with."""
        from .params import fleet_drag_accel
        return fleet_drag_accel(self.fleet_get()[0], v)

    # ---- the sensor: noise, bias, latency and dropout between the plant and the controller
    def sensor_start(self, sensors, seed=0, index0=0, period0=0, depth=1, judge=0):
        """Measure through sensors [B] of params.SENSOR_DTYPE (params.sensor_defaults / sensor_sample build them) in every period of
        sim_steps / sim_control_periods from now on: the step, the recorder, the black box and the exploration see the delivered
        measurement, not the plant state.  seed and index0 (the global index of quadrotor 0) select the draws, period0 is the first
        sensor period, depth (1..32) the ring that latency reads from (every delay <= depth - 1); judge: params.SENSOR_JUDGE_MEASURED
        (score and black box judge what the controller saw) or SENSOR_JUDGE_TRUTH (they read the true plant state).  Calling it again
        replaces the sensor.  step() takes the caller's measurement: a host loop is sensor_sample -> step -> sim_plant_period."""
        from .params import SENSOR_DTYPE
        sensors = np.ascontiguousarray(sensors)
        if sensors.dtype != SENSOR_DTYPE or sensors.shape != (self.B,):
            raise ValueError(f"sensors must be a [B={self.B}] array of params.SENSOR_DTYPE")
        self._check(self.lib.mpcq_sensor_start(self.h, sensors.ctypes.data_as(ctypes.c_void_p), SENSOR_DTYPE.itemsize, int(seed) & (2 ** 64 - 1),
                                               int(index0), int(period0), int(depth), int(judge)))

    def sensor_get(self):
        """(the delivered measurement [B, 13], its age in periods [B], the number of the next sensor period)."""
        x, age, period = np.zeros((self.B, NX)), np.zeros(self.B, np.int32), ctypes.c_int64()
        self._check(self.lib.mpcq_sensor_get(self.h, _lib.d(x), _lib.i(age), ctypes.byref(period)))
        return x, age, period.value

    def sensor_sample(self):
        """One sensor period on the current plant state: the delivered measurement [B, 13] (what the step of that period of sim_steps
        would solve from)."""
        x = np.zeros((self.B, NX))
        self._check(self.lib.mpcq_sensor_sample(self.h, _lib.d(x)))
        return x

    def sensor_stop(self):
        """Back to the identity: the step of sim_steps solves from the plant state."""
        self._check(self.lib.mpcq_sensor_stop(self.h))

    # ---- exploration: the limits of the next mission leg from the envelope of body velocities the quadrotor has flown
    def explore_start(self, rules, leg_mask=None, env=None, samples=None):
        """Explore with the mission that is set (mpcq_explore_start): in the period a flight ends, v_max and a_max of the quadrotor's
        next leg are set on the device from its envelope by its rule (params.explore_velocity is the host form).  rules [B] of
        params.EXPLORE_RULE_DTYPE (params.explore_rules builds them); leg_mask [B, L] (None: every leg is explored); env [B, 3, 2] with
        samples [B]: the envelope to start from (a checkpoint's explore_get), None for the empty one.  Calling it again replaces rules,
        mask and envelope and empties the log; mission_set* and mission_stop end the exploration."""
        from .params import EXPLORE_RULE_DTYPE
        L = getattr(self, "_mission_legs", None)
        if L is None:
            raise _lib.MpcqError("explore_start needs mission_set first")
        rules = np.ascontiguousarray(rules)
        if rules.dtype != EXPLORE_RULE_DTYPE or rules.shape != (self.B,):
            raise ValueError(f"rules must be a [B={self.B}] array of params.EXPLORE_RULE_DTYPE")
        if leg_mask is not None:
            leg_mask = np.ascontiguousarray(np.asarray(leg_mask) != 0, dtype=np.uint8)
            if leg_mask.shape != (self.B, L):
                raise ValueError(f"leg_mask must be [B={self.B}, L={L}]")
        env = self._f(env, (self.B, 3, 2))
        samples = None if samples is None else np.ascontiguousarray(samples, dtype=np.int64).reshape(self.B)
        self._check(self.lib.mpcq_explore_start(self.h, rules.ctypes.data_as(ctypes.c_void_p), EXPLORE_RULE_DTYPE.itemsize,
                                                None if leg_mask is None else leg_mask.ctypes.data_as(ctypes.c_void_p), _lib.d(env), _lib.l(samples)))

    def explore_get(self):
        """dict(env [B, 3, 2]: min and max of v_body per axis (zeros while samples == 0), samples [B], leg_limits [B, L, 3]: (explored,
        v_max, a_max) of every leg the exploration has set, NaN elsewhere)."""
        L = getattr(self, "_mission_legs", None) or 0
        out = dict(env=np.zeros((self.B, 3, 2)), samples=np.zeros(self.B, np.int64), leg_limits=np.zeros((self.B, L, 3)))
        self._check(self.lib.mpcq_explore_get(self.h, _lib.d(out["env"]), _lib.l(out["samples"]), _lib.d(out["leg_limits"])))
        return out

    def explore_stop(self):
        """Exploration off; the mission flies on with the limits its table holds now."""
        self._check(self.lib.mpcq_explore_stop(self.h))

    def set_reference(self, yref, yrefN):
        yref = self._f(yref, (self.B, self.N, NY))
        yrefN = self._f(yrefN, (self.B, NX))
        self._check(self.lib.mpcq_set_reference(self.h, _lib.d(yref), _lib.d(yrefN)))

    def set_params(self, mu):
        mu = self._f(mu, (self.B, 3 * self.nb))
        self._check(self.lib.mpcq_set_params(self.h, _lib.d(mu)))

    def get_state(self):
        B, N, nb = self.B, self.N, self.nb
        s = dict(X=np.zeros((B, N + 1, NX)), U=np.zeros((B, N, NU)), mu=np.zeros((B, 3, nb)),
                 C=np.zeros((B, 3, nb, nb)), x_pred_prev=np.zeros((B, NX)),
                 has_prev=np.zeros(B, np.int32), idx=np.zeros(B, np.int32))
        self._check(self.lib.mpcq_get_state(self.h, _lib.d(s["X"]), _lib.d(s["U"]), _lib.d(s["mu"]), _lib.d(s["C"]),
                                            _lib.d(s["x_pred_prev"]), _lib.i(s["has_prev"]), _lib.i(s["idx"])))
        return s

    def set_state(self, X=None, U=None, mu=None, C=None, x_pred_prev=None, has_prev=None, idx=None):
        g = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.int32)
        X, U, mu, C, xp = (self._f(a) for a in (X, U, mu, C, x_pred_prev))
        hp, ix = g(has_prev), g(idx)
        self._check(self.lib.mpcq_set_state(self.h, _lib.d(X), _lib.d(U), _lib.d(mu), _lib.d(C), _lib.d(xp),
                                            _lib.i(hp), _lib.i(ix)))

    # ---- explicit path (acados-style set / solve / get)
    def solve(self, x0):
        x0 = self._f(x0, (self.B, NX))
        self._check(self.lib.mpcq_solve(self.h, _lib.d(x0)))

    def get_x(self, stage):
        out = np.zeros((self.B, NX))
        self._check(self.lib.mpcq_get_x(self.h, stage, _lib.d(out)))
        return out

    def get_u(self, stage):
        out = np.zeros((self.B, NU))
        self._check(self.lib.mpcq_get_u(self.h, stage, _lib.d(out)))
        return out

    def get_cost(self):
        out = np.zeros(self.B)
        self._check(self.lib.mpcq_get_cost(self.h, _lib.d(out)))
        return out

    def get_status(self):
        out = np.zeros(self.B, np.int32)
        self._check(self.lib.mpcq_get_status(self.h, _lib.i(out)))
        return out

    def get_qp_iter(self):
        out = np.zeros(self.B, np.int32)
        self._check(self.lib.mpcq_get_qp_iter(self.h, _lib.i(out)))
        return out

    def get_qp_work(self):
        """(factorisations, vector sweeps) the last solve of every quadrotor executed."""
        out = np.zeros(self.B, np.int32)
        self._check(self.lib.mpcq_get_qp_work(self.h, _lib.i(out)))
        return out & 0x7FFF, (out >> 16) & 0x7FF

    def get_qp_float_iterations(self):
        """fp64 instances: how many interior-point iterations of the last solve ran in float (bits 27..31 of mpcq_get_qp_work)."""
        out = np.zeros(self.B, np.int32)
        self._check(self.lib.mpcq_get_qp_work(self.h, _lib.i(out)))
        return (out.view(np.uint32) >> 27).astype(np.int32)

    def get_qp_float_breakdown(self):
        """fp64 instances: True where the float interior point of the last (fallback) solve broke down and the double one ran instead."""
        out = np.zeros(self.B, np.int32)
        self._check(self.lib.mpcq_get_qp_work(self.h, _lib.i(out)))
        return (out & 0x8000) != 0

    def get_block_order(self):
        """Launch order of the last lockstep period: workgroup p ran quadrotor out[p] (identity when unused)."""
        out = np.zeros(self.B, np.int32)
        self._check(self.lib.mpcq_get_block_order(self.h, _lib.i(out)))
        return out

    def get_groups(self):
        """Groups mpcq_sim_steps runs the batch in (mpcq_tuning.groups resolved; 1 = one launch per period over the whole batch)."""
        out = ctypes.c_int32()
        self._check(self.lib.mpcq_get_groups(self.h, ctypes.byref(out)))
        return out.value

    def get_time(self):
        t = ctypes.c_double()
        self._check(self.lib.mpcq_get_stats(self.h, ctypes.byref(t)))
        return t.value

    def predict_nominal(self, x, u, dt):
        x, u = self._f(x, (self.B, NX)), self._f(u, (self.B, NU))
        out = np.zeros((self.B, NX))
        self._check(self.lib.mpcq_predict_nominal(self.h, _lib.d(x), _lib.d(u), float(dt), _lib.d(out)))
        return out

    def rgp_regress(self, v_body, a_drag):
        vb, ad = self._f(v_body, (self.B, 3)), self._f(a_drag, (self.B, 3))
        self._check(self.lib.mpcq_rgp_regress(self.h, _lib.d(vb), _lib.d(ad)))

    def get_rgp(self):
        mu = np.zeros((self.B, 3, self.nb))
        C = np.zeros((self.B, 3, self.nb, self.nb))
        self._check(self.lib.mpcq_get_rgp(self.h, _lib.d(mu), _lib.d(C)))
        return mu, C

    def rgp_predict(self, xq, var=True, per_quad=False):
        """Posterior of every quadrotor's drag model at query points xq [3,M] (one grid per axis, shared by the batch) or, with
        per_quad, [B,3,M]: mean [B,3,M], and with var the variance [B,3,M] (as computed: take np.sqrt for the reference's std)."""
        xq = self._f(xq)
        if xq.shape[:-1] != ((self.B, 3) if per_quad else (3,)):
            raise ValueError(f"xq must be [B={self.B}, 3, M]" if per_quad else "xq must be [3, M]")
        M = xq.shape[-1]
        mean = np.zeros((self.B, 3, M))
        v = np.zeros((self.B, 3, M)) if var else None
        self._check(self.lib.mpcq_rgp_predict(self.h, _lib.d(xq), M, int(bool(per_quad)), _lib.d(mean), _lib.d(v)))
        return (mean, v) if var else mean

    def record_predict(self, xq, rows=None, var=True):
        """rgp_predict for the recorded rows `rows` = (row0, nrows) (None: all recorded so far) of the active recording, evaluated from
        the device buffers in place: mean [count,R,3,M] (and variance) for the recorded quadrotors in the order of record_start."""
        xq = self._f(xq)
        if xq.ndim != 2 or xq.shape[0] != 3:
            raise ValueError("xq must be [3, M]")
        recorded = self.record_info()[0]
        row0, nrows = (0, recorded) if rows is None else (int(rows[0]), int(rows[1]))
        n, M = len(self._rec["quads"]), xq.shape[1]
        mean = np.zeros((n, nrows, 3, M))
        v = np.zeros((n, nrows, 3, M)) if var else None
        if rows is not None or nrows > 0:      # (nothing recorded yet: empty arrays)
            self._check(self.lib.mpcq_record_predict(self.h, _lib.d(xq), M, row0, nrows, _lib.d(mean), _lib.d(v)))
        return (mean, v) if var else mean

    # ---- training on the device: all samples of a stream in one launch
    def _train_call(self, S, mode, basis, theta, pair_next, call):
        """spec and output arrays of a training call; call(spec, out) -> rc"""
        if mode not in _lib.TRAIN_MODES:
            raise ValueError(f"mode must be one of {sorted(_lib.TRAIN_MODES)}")
        if (basis is None) != (theta is None):
            raise ValueError("basis and theta go together (both None: the engine's own model)")
        keep = []
        if basis is None:
            n = self.nb
        else:
            basis = np.ascontiguousarray(basis, dtype=np.float64).reshape(3, -1)
            th = np.asarray(theta, dtype=np.float64)
            theta = np.ascontiguousarray(np.tile(th, (3, 1)) if th.shape == (3,) else th.reshape(3, 3))
            n = basis.shape[1]
            keep = [basis, theta]
        spec = _lib.TrainSpec(mode=_lib.TRAIN_MODES[mode], pair_next=int(bool(pair_next)), nb=0 if basis is None else n,
                              basis=_lib.d(basis), theta=_lib.d(theta))
        res = dict(mu_g=np.zeros((S, 3, n)), C_g=np.zeros((S, 3, n, n)))
        if mode == "learn":
            res.update(mu_eta=np.zeros((S, 3, 3)), C_eta=np.zeros((S, 3, 3, 3)), K_x_inv=np.zeros((S, 3, n, n)))
        out = _lib.TrainOut(mu=_lib.d(res["mu_g"]), C=_lib.d(res["C_g"]), mu_eta=_lib.d(res.get("mu_eta")), C_eta=_lib.d(res.get("C_eta")),
                            Kx_inv=_lib.d(res.get("K_x_inv")))
        self._check(call(ctypes.byref(spec), ctypes.byref(out)))
        del keep
        return res

    def rgp_train(self, v_body, a_drag, mode="regress", basis=None, theta=None, pair_next=False):
        """Train S x 3 drag models on sample streams v_body, a_drag [S,T,3] in one launch: mode "regress" (RGP.regress over all
        samples, fixed hyper-parameters) or "learn" (RGP.learn, what Learner.step does sample by sample).  basis [3,nb] and theta
        (3 values or [3,3]) name another model than the engine's own (None, None); pair_next pairs v_body[t] with a_drag[t+1] (the
        reference's offline loader).  Returns the keys of Learner.get(): mu_g [S,3,nb], C_g [S,3,nb,nb], and for "learn" mu_eta,
        C_eta, K_x_inv.  A "regress" result on the engine's own model loads with set_state(mu=, C=)."""
        v = np.ascontiguousarray(v_body, dtype=np.float64)
        a = np.ascontiguousarray(a_drag, dtype=np.float64)
        if v.ndim != 3 or v.shape[2] != 3 or a.shape != v.shape:
            raise ValueError("v_body and a_drag must both be [S, T, 3]")
        S, T = v.shape[0], v.shape[1]
        return self._train_call(S, mode, basis, theta, pair_next,
                                lambda sp, out: self.lib.mpcq_rgp_train(self.h, sp, _lib.d(v), _lib.d(a), S, T, out))

    def record_train(self, rows=None, mode="regress", basis=None, theta=None, pair_next=False):
        """rgp_train on the recorded rows `rows` = (row0, nrows) (None: all recorded so far) of the active recording's v_body / a_drag,
        read from the device buffer in place, for the recorded quadrotors in the order of record_start."""
        rec = getattr(self, "_rec", None)
        recorded = self.record_info()[0]   # (raises without an active recording)
        row0, nrows = (0, recorded) if rows is None else (int(rows[0]), int(rows[1]))
        return self._train_call(len(rec["quads"]), mode, basis, theta, pair_next,
                                lambda sp, out: self.lib.mpcq_record_train(self.h, sp, row0, nrows, out))

    # ---- fused path
    def step(self, x_meas):
        x = self._f(x_meas, (self.B, NX))
        w = np.zeros((self.B, NU))
        xp = np.zeros((self.B, NX))
        self._check(self.lib.mpcq_step(self.h, _lib.d(x), _lib.d(w), _lib.d(xp)))
        self._periods += 1
        return w, xp

    def sim_reset(self, x0):
        x0 = self._f(x0, (self.B, NX))
        self._check(self.lib.mpcq_sim_reset(self.h, _lib.d(x0)))

    def sim_steps(self, K, n_sub, sim_dt=5e-3):
        self._check(self.lib.mpcq_sim_steps(self.h, int(K), int(n_sub), float(sim_dt)))
        self._periods += max(int(K), 0)

    def sim_run(self, K, n_sub, sim_dt=5e-3):
        """K closed-loop periods in one launch, every instance advancing on its own (same results as sim_steps)."""
        self._check(self.lib.mpcq_sim_run(self.h, int(K), int(n_sub), float(sim_dt)))

    def sim_get_state(self):
        x = np.zeros((self.B, NX))
        w = np.zeros((self.B, NU))
        self._check(self.lib.mpcq_sim_get_state(self.h, _lib.d(x), _lib.d(w)))
        return x, w

    # ---- outputs of the loop body beyond w (a4, a9)
    def get_command(self):
        """(rotor_thrusts [B,4], collective_thrust [B], bodyrates [B,3]) of publish_control_gazebo."""
        rotor, coll, rates = np.zeros((self.B, NU)), np.zeros(self.B), np.zeros((self.B, 3))
        self._check(self.lib.mpcq_get_command(self.h, _lib.d(rotor), _lib.d(coll), _lib.d(rates)))
        return rotor, coll, rates

    def get_finished(self):
        out = np.zeros(self.B, np.int32)
        self._check(self.lib.mpcq_get_finished(self.h, _lib.i(out)))
        return out

    def get_reference_chunk(self):
        out = np.zeros((self.B, self.N, NX))
        self._check(self.lib.mpcq_get_reference_chunk(self.h, _lib.d(out)))
        return out

    def plant_substeps(self, control_dt, sim_dt=5e-3):
        return int(self.lib.mpcq_plant_substeps(float(control_dt), float(sim_dt)))

    def sim_plant_period(self, w, control_dt, sim_dt=5e-3):
        """Advance the plant state by the reference's float-accumulated substep loop; returns the substep count."""
        w = self._f(w, (self.B, NU))
        n = ctypes.c_int32()
        self._check(self.lib.mpcq_sim_plant_period(self.h, _lib.d(w), float(control_dt), float(sim_dt), ctypes.byref(n)))
        return n.value

    def sim_control_periods(self, K, control_dt, sim_dt=5e-3):
        n = ctypes.c_int32()
        self._check(self.lib.mpcq_sim_control_periods(self.h, int(K), float(control_dt), float(sim_dt), ctypes.byref(n)))
        self._periods += max(int(K), 0)
        return n.value

    def step_device_async(self, d_x_meas: int, d_w_out: int = 0):
        """Fused step on float64 device buffers (raw device addresses); asynchronous on the engine's stream."""
        self._check(self.lib.mpcq_step_device_async(self.h, ctypes.c_void_p(d_x_meas), ctypes.c_void_p(d_w_out or None)))
        self._periods += 1

    def synchronize(self):
        self._check(self.lib.mpcq_synchronize(self.h))

    def get_solver_state(self):
        s = dict(qp_iter=np.zeros(self.B, np.int32), stats=np.zeros((self.B, 4)), finished=np.zeros(self.B, np.int32))
        self._check(self.lib.mpcq_get_solver_state(self.h, _lib.i(s["qp_iter"]), _lib.d(s["stats"]), _lib.i(s["finished"])))
        return s

    def set_solver_state(self, qp_iter=None, stats=None, finished=None):
        g = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.int32)
        q, f, st = g(qp_iter), g(finished), self._f(stats)
        self._check(self.lib.mpcq_set_solver_state(self.h, _lib.i(q), _lib.d(st), _lib.i(f)))

    def get_kernel_time_minmax(self):
        a, b = ctypes.c_double(), ctypes.c_double()
        self._check(self.lib.mpcq_get_kernel_time_minmax(self.h, ctypes.byref(a), ctypes.byref(b)))
        return a.value, b.value

    def get_kernel_time(self):
        t = ctypes.c_double()
        n = ctypes.c_int32()
        self._check(self.lib.mpcq_get_kernel_time(self.h, ctypes.byref(t), ctypes.byref(n)))
        return t.value, n.value

    def get_tracking_stats(self):
        out = np.zeros(5)
        self._check(self.lib.mpcq_get_tracking_stats(self.h, _lib.d(out)))
        return out

    # ---- multi-GPU statistics
    def comm_unique_id(self) -> bytes:
        buf = ctypes.create_string_buffer(128)
        self._check(self.lib.mpcq_comm_unique_id(buf))
        return buf.raw

    def comm_init(self, rank, nranks, uid: bytes):
        buf = ctypes.create_string_buffer(uid, 128)
        self._check(self.lib.mpcq_comm_init(self.h, rank, nranks, buf))

    def comm_share(self, owner: "Engine"):
        """Reduce over the communicator another engine of this process initialised (one communicator per rank)."""
        self._check(self.lib.mpcq_comm_share(self.h, owner.h))

    def allreduce_tracking_stats(self):
        out = np.zeros(5)
        self._check(self.lib.mpcq_allreduce_tracking_stats(self.h, _lib.d(out)))
        return out


class Learner:
    """batch x 3 recursive GPs with hyper-parameter learning on the device (RGP.learn, src/gp/RGP.py:332-505);
    the offline estimator of the reference, not part of the control step."""

    def __init__(self, batch, basis, theta, device=0, lib_path=None):
        self.lib = _lib.load(lib_path)
        self.basis = np.ascontiguousarray(basis, dtype=np.float64).reshape(3, -1)
        th = np.asarray(theta, dtype=np.float64)
        self.theta = np.ascontiguousarray(np.tile(th, (3, 1)) if th.shape == (3,) else th.reshape(3, 3))
        self.B, self.nb = int(batch), self.basis.shape[1]
        h = ctypes.c_void_p()
        self._check(self.lib.mpcq_learn_create(self.B, self.nb, _lib.d(self.basis), _lib.d(self.theta), int(device), ctypes.byref(h)))
        self.h = h

    def _check(self, rc):
        if rc != 0:
            raise _lib.MpcqError(f"mpcq error {rc}: {self.lib.mpcq_learn_last_error().decode()}")

    def step(self, v_body, a_drag):
        s = np.ascontiguousarray(v_body, dtype=np.float64).reshape(self.B, 3)
        y = np.ascontiguousarray(a_drag, dtype=np.float64).reshape(self.B, 3)
        self._check(self.lib.mpcq_learn_step(self.h, _lib.d(s), _lib.d(y)))

    def get(self):
        B, n = self.B, self.nb
        out = dict(mu_g=np.zeros((B, 3, n)), C_g=np.zeros((B, 3, n, n)), mu_eta=np.zeros((B, 3, 3)), C_eta=np.zeros((B, 3, 3, 3)),
                   K_x_inv=np.zeros((B, 3, n, n)))
        self._check(self.lib.mpcq_learn_get(self.h, _lib.d(out["mu_g"]), _lib.d(out["C_g"]), _lib.d(out["mu_eta"]), _lib.d(out["C_eta"]),
                                            _lib.d(out["K_x_inv"])))
        return out

    def close(self):
        if getattr(self, "h", None):
            self.lib.mpcq_learn_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

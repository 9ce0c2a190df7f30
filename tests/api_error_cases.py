"""The table behind tests/test_api_errors.py and tests/golden/make_api_errors_golden.py: invalid calls of the C ABI against a tiny engine
(B = 3, N = 4, nb = 2; nb = 0 for the "no RGP" cases), each with the state it is made in.  run_cases() returns, per case, the return code
and the text of mpcq_last_error() ("" after a call that succeeds: the text is stale then).

A case is (id, state, call).  `state` names what is set up on a fresh engine, in this order: "nb0" (an engine without RGP), "traj"
(mpcq_set_trajectories), "sim" (mpcq_sim_reset), "rec" / "rec_mu" / "rec_x" (a recording of every field / without MPCQ_RECORD_RGP_C /
of x_odom only), "mission", "explore", "score", "fleet".  No case launches the step kernel.  Cases whose id ends in a "+"-joined pair
break two rules at once: they pin the order of the checks.

Not in the table: errors that need a failed allocation or a device error, and the two "queue too large (B x L x n_wp)" checks behind the
per-leg loop, which need a host array of B x L > 1e8 legs to reach."""
import ctypes

import numpy as np

from mpc_quad_ros_amd import _lib
from mpc_quad_ros_amd.engine import Engine
from mpc_quad_ros_amd.params import EXPLORE_RULE_DTYPE, PLANT_DTYPE, EngineConfig, explore_rules, fleet_defaults, hummingbird, rgp_basis_linspace

B, N, NB, TMAX = 3, 4, 2, 6
REC_ALL, REC_X, REC_MU, REC_C, REC_DRAG, REC_SOLVER = 511, 1, 64, 128, 32, 256
INF, NAN = float("inf"), float("nan")


def config(nb):
    kw = dict(basis=rgp_basis_linspace(12.0, nb)) if nb else {}
    return EngineConfig(batch=B, N=N, T=1.0, quad=hummingbird(), nb=nb, dt_pred=0.01, **kw)


class Ctx:
    """A fresh engine in `state` and the arguments the calls are made of."""

    def __init__(self, lib_path, state):
        self.nb = 0 if "nb0" in state else NB
        self.cfg = config(self.nb)
        self.e = Engine(self.cfg, lib_path=lib_path)
        self.lib, self.h = self.e.lib, self.e.h
        self.keep = []   # arrays a call points into
        for s in state:
            if s != "nb0":
                rc = getattr(self, "setup_" + s)()
                assert rc == 0, (state, s, rc, self.lib.mpcq_last_error().decode())

    # ---- arguments
    def d(self, *shape, fill=0.0):
        a = np.full(shape, fill, np.float64)
        self.keep.append(a)
        return _lib.d(a)

    def i(self, values):
        a = np.ascontiguousarray(values, dtype=np.int32)
        self.keep.append(a)
        return _lib.i(a)

    def l(self, values):
        a = np.ascontiguousarray(values, dtype=np.int64)
        self.keep.append(a)
        return _lib.l(a)

    def opts(self, **over):
        o = _lib.nl_options(over)
        self.keep.append(o)
        return ctypes.byref(o)

    def legs(self, L=1, **over):
        """[B, L] circle legs (v_max 2, a_max 2, radius 1); over: field -> (b, l, value)"""
        a = (_lib.Leg * (B * L))()
        for k in range(B * L):
            a[k].kind, a[k].reserved, a[k].v_max, a[k].a_max, a[k].radius = 1, 0, 2.0, 2.0, 1.0
        for name, (b, l, v) in over.items():
            setattr(a[b * L + l], name, v)
        self.keep.append(a)
        return a

    def rules(self, **over):
        """over: field -> (b, value)"""
        r = explore_rules(B)
        for name, (b, v) in over.items():
            r[name][b] = v
        self.keep.append(r)
        return r.ctypes.data_as(ctypes.c_void_p)

    def plants(self, **over):
        """over: field -> (b, index or None, value)"""
        p = fleet_defaults(self.cfg, B)
        for name, (b, k, v) in over.items():
            if k is None:
                p[name][b] = v
            else:
                p[name][b, k] = v
        self.keep.append(p)
        return p.ctypes.data_as(ctypes.c_void_p)

    def spec(self, mode=1, pair_next=0, nb=0, basis=False, theta=None):
        th = None if theta is None else self.d(9, fill=theta)
        s = _lib.TrainSpec(mode, pair_next, nb, self.d(3, max(nb, 1)) if basis else None, th)
        self.keep.append(s)
        return ctypes.byref(s)

    def out(self, mu=True, mu_eta=False):
        o = _lib.TrainOut(self.d(B * 3 * 64) if mu else None, None, self.d(B * 9) if mu_eta else None, None, None)
        self.keep.append(o)
        return ctypes.byref(o)

    # ---- states
    def setup_traj(self):
        return self.lib.mpcq_set_trajectories(self.h, self.d(B, TMAX, 13), self.i([TMAX] * B), TMAX)

    def setup_sim(self):
        return self.lib.mpcq_sim_reset(self.h, self.d(B, 13))

    def setup_rec(self, fields=REC_ALL):
        return self.lib.mpcq_record_start(self.h, None, 0, fields, 1, 4)

    def setup_rec_mu(self):
        return self.setup_rec(REC_ALL & ~REC_C & ~REC_DRAG & ~REC_SOLVER)

    def setup_rec_x(self):
        return self.setup_rec(REC_X)

    def setup_mission(self):
        return self.lib.mpcq_mission_set(self.h, self.d(B, 1, 1, 3), 1, 1, 2.0, 2.0, 4, 0.01, 0, None, None)

    def setup_explore(self):
        return self.lib.mpcq_explore_start(self.h, self.rules(), EXPLORE_RULE_DTYPE.itemsize, None, None, None)

    def setup_score(self):
        return self.lib.mpcq_score_start(self.h, 1, 0)

    def setup_fleet(self):
        return self.lib.mpcq_fleet_set(self.h, self.plants(), PLANT_DTYPE.itemsize, 0)

    # ---- the calls with most of their arguments valid
    def replan(self, wp=True, n_wp=1, v=2.0, a=2.0, order=4, dt=0.01, start=True):
        return self.lib.mpcq_replan(self.h, self.d(B, 3) if start else None, self.d(B, 8, 3) if wp else None, n_wp, v, a, order, dt, None, None)

    def replan_nl(self, wp=True, n_wp=1, v=2.0, a=2.0, order=3, dt=0.01, start=True, opts=None):
        return self.lib.mpcq_replan_nonlinear(self.h, self.d(B, 3) if start else None, self.d(B, 8, 3) if wp else None, n_wp, v, a, order, dt, None, None,
                                              opts, None, None, None)

    def circle(self, radius=True, kind=0, dt=0.01, t_max=10.0, start=True):
        return self.lib.mpcq_replan_circle(self.h, self.d(B, 3) if start else None, self.d(B, fill=1.0) if radius else None, self.d(B, fill=1.0), kind, dt,
                                           t_max, None, None)

    def replace(self, idx=(0,), count=None, lens=(TMAX,), null=False):
        return self.lib.mpcq_replace_trajectories(self.h, None if null else self.i(list(idx) + [0] * B), len(idx) if count is None else count,
                                                  self.d(B + 1, TMAX, 13), self.i(list(lens) + [1] * B))

    def mission_set(self, wp=True, L=1, n_wp=1, v=2.0, a=2.0, order=4, dt=0.01, nonlinear=0, opts=None, leg0=None):
        return self.lib.mpcq_mission_set(self.h, self.d(B, 2, 8, 3) if wp else None, L, n_wp, v, a, order, dt, nonlinear, opts,
                                         None if leg0 is None else self.i(leg0))

    def set_legs(self, legs="default", wp=False, L=1, n_wp=0, order=4, dt=0.01, nonlinear=0, opts=None, leg0=None):
        legs = self.legs(max(L, 1)) if isinstance(legs, str) else legs
        return self.lib.mpcq_mission_set_legs(self.h, legs, self.d(B, 2, 8, 3) if wp else None, L, n_wp, order, dt, nonlinear, opts,
                                              None if leg0 is None else self.i(leg0))

    def explore(self, rules="default", size=EXPLORE_RULE_DTYPE.itemsize, env=False, samples=None):
        return self.lib.mpcq_explore_start(self.h, self.rules() if isinstance(rules, str) else rules, size, None, self.d(B, 3, 2) if env else None,
                                           None if samples is None else self.l(samples))

    def record_start(self, quads=None, count=0, fields=REC_X, every=1, capacity=4):
        return self.lib.mpcq_record_start(self.h, None if quads is None else self.i(quads), count, fields, every, capacity)

    def rgp_predict(self, xq=True, M=2, per_quad=0, mean=True):
        return self.lib.mpcq_rgp_predict(self.h, self.d(3, 8) if xq else None, M, per_quad, self.d(B, 3, 8) if mean else None, None)

    def record_predict(self, xq=True, M=2, row0=0, nrows=1, mean=True, var=False):
        return self.lib.mpcq_record_predict(self.h, self.d(3, 8) if xq else None, M, row0, nrows, self.d(4, B, 3, 8) if mean else None,
                                            self.d(4, B, 3, 8) if var else None)

    def rgp_train(self, spec="default", out="default", samples=True, S=1, T=2):
        return self.lib.mpcq_rgp_train(self.h, self.spec() if isinstance(spec, str) else spec, self.d(2, 4, 3) if samples else None, self.d(2, 4, 3), S, T,
                                       self.out() if isinstance(out, str) else out)

    def record_train(self, spec="default", out="default", row0=0, nrows=1):
        return self.lib.mpcq_record_train(self.h, self.spec() if isinstance(spec, str) else spec, row0, nrows, self.out() if isinstance(out, str) else out)

    def fleet_set(self, plants="default", size=PLANT_DTYPE.itemsize, period0=0):
        return self.lib.mpcq_fleet_set(self.h, self.plants() if isinstance(plants, str) else plants, size, period0)


T, TS = ("traj",), ("traj", "sim")
BAD_OPTS = dict(max_evaluations=0)

CASES = [
    # ---- periods without trajectories
    ("step/no_traj", (), lambda c: c.lib.mpcq_step(c.h, c.d(B, 13), c.d(B, 4), None)),
    ("step_device/no_traj", (), lambda c: c.lib.mpcq_step_device_async(c.h, 1, None)),
    ("sim_steps/no_traj", (), lambda c: c.lib.mpcq_sim_steps(c.h, 1, 2, 5e-3)),
    ("sim_control_periods/no_traj", (), lambda c: c.lib.mpcq_sim_control_periods(c.h, 1, 0.01, 5e-3, None)),
    ("sim_control_periods/bad_dt+no_traj", (), lambda c: c.lib.mpcq_sim_control_periods(c.h, 1, 0.01, 0.0, None)),
    ("sim_plant_period/bad_dt", T, lambda c: c.lib.mpcq_sim_plant_period(c.h, None, -1.0, 5e-3, None)),
    ("get_reference_chunk/no_traj", (), lambda c: c.lib.mpcq_get_reference_chunk(c.h, c.d(B, N, 13))),
    ("get_trajectories/no_traj", (), lambda c: c.lib.mpcq_get_trajectories(c.h, None, None)),
    # ---- mpcq_sim_run
    ("sim_run/no_traj", (), lambda c: c.lib.mpcq_sim_run(c.h, 1, 2, 5e-3)),
    ("sim_run/recording", T + ("rec_x",), lambda c: c.lib.mpcq_sim_run(c.h, 1, 2, 5e-3)),
    ("sim_run/exploring", T + ("mission", "explore"), lambda c: c.lib.mpcq_sim_run(c.h, 1, 2, 5e-3)),
    ("sim_run/mission", T + ("mission",), lambda c: c.lib.mpcq_sim_run(c.h, 1, 2, 5e-3)),
    ("sim_run/score", T + ("score",), lambda c: c.lib.mpcq_sim_run(c.h, 1, 2, 5e-3)),
    ("sim_run/fleet", T + ("fleet",), lambda c: c.lib.mpcq_sim_run(c.h, 1, 2, 5e-3)),
    ("sim_run/no_traj+recording", ("rec_x",), lambda c: c.lib.mpcq_sim_run(c.h, 1, 2, 5e-3)),
    ("sim_run/recording+score", T + ("rec_x", "score"), lambda c: c.lib.mpcq_sim_run(c.h, 1, 2, 5e-3)),
    ("sim_run/mission+score", T + ("mission", "score"), lambda c: c.lib.mpcq_sim_run(c.h, 1, 2, 5e-3)),
    ("sim_run/score+fleet", T + ("score", "fleet"), lambda c: c.lib.mpcq_sim_run(c.h, 1, 2, 5e-3)),
    ("sim_run/everything", T + ("rec_x", "mission", "explore", "score", "fleet"), lambda c: c.lib.mpcq_sim_run(c.h, 1, 2, 5e-3)),
    # ---- mpcq_replan
    ("replan/null_wp", TS, lambda c: c.replan(wp=False)),
    ("replan/n_wp_0", TS, lambda c: c.replan(n_wp=0)),
    ("replan/n_wp_8", TS, lambda c: c.replan(n_wp=8)),
    ("replan/v_max_0", TS, lambda c: c.replan(v=0.0)),
    ("replan/dt_nan", TS, lambda c: c.replan(dt=NAN)),
    ("replan/order_1", TS, lambda c: c.replan(order=1)),
    ("replan/order_5", TS, lambda c: c.replan(order=5)),
    ("replan/no_traj", (), lambda c: c.replan()),
    ("replan/no_sim", T, lambda c: c.replan(start=False)),
    ("replan/null_wp+n_wp_0", TS, lambda c: c.replan(wp=False, n_wp=0)),
    ("replan/n_wp_0+v_max_0", TS, lambda c: c.replan(n_wp=0, v=0.0)),
    ("replan/v_max_0+order_5", TS, lambda c: c.replan(v=0.0, order=5)),
    ("replan/order_5+no_traj", (), lambda c: c.replan(order=5)),
    ("replan/no_traj+no_sim", (), lambda c: c.replan(start=False)),
    # ---- mpcq_replan_nonlinear
    ("replan_nl/null_wp", TS, lambda c: c.replan_nl(wp=False)),
    ("replan_nl/n_wp_0", TS, lambda c: c.replan_nl(n_wp=0)),
    ("replan_nl/n_wp_8", TS, lambda c: c.replan_nl(n_wp=8)),
    ("replan_nl/v_max_inf", TS, lambda c: c.replan_nl(v=INF)),
    ("replan_nl/a_max_neg", TS, lambda c: c.replan_nl(a=-1.0)),
    ("replan_nl/order_1", TS, lambda c: c.replan_nl(order=1)),
    ("replan_nl/bad_opts", TS, lambda c: c.replan_nl(opts=c.opts(**BAD_OPTS))),
    ("replan_nl/no_traj", (), lambda c: c.replan_nl()),
    ("replan_nl/no_sim", T, lambda c: c.replan_nl(start=False)),
    ("replan_nl/n_wp_8+v_max_inf", TS, lambda c: c.replan_nl(n_wp=8, v=INF)),
    ("replan_nl/v_max_inf+order_1", TS, lambda c: c.replan_nl(v=INF, order=1)),
    ("replan_nl/order_1+bad_opts", TS, lambda c: c.replan_nl(order=1, opts=c.opts(**BAD_OPTS))),
    ("replan_nl/bad_opts+no_traj", (), lambda c: c.replan_nl(opts=c.opts(**BAD_OPTS))),
    ("replan_nl/no_traj+no_sim", (), lambda c: c.replan_nl(start=False)),
    # ---- mpcq_replan_circle
    ("circle/null_radius", TS, lambda c: c.circle(radius=False)),
    ("circle/kind_7", TS, lambda c: c.circle(kind=7)),
    ("circle/dt_0", TS, lambda c: c.circle(dt=0.0)),
    ("circle/dt_inf", TS, lambda c: c.circle(dt=INF)),
    ("circle/accelerating_t_max_0", TS, lambda c: c.circle(kind=2, t_max=0.0)),
    ("circle/no_traj", (), lambda c: c.circle()),
    ("circle/no_sim", T, lambda c: c.circle(start=False)),
    ("circle/null_radius+kind_7", TS, lambda c: c.circle(radius=False, kind=7)),
    ("circle/kind_7+dt_0", TS, lambda c: c.circle(kind=7, dt=0.0)),
    ("circle/dt_0+t_max_0", TS, lambda c: c.circle(kind=2, dt=0.0, t_max=0.0)),
    ("circle/t_max_0+no_traj", (), lambda c: c.circle(kind=2, t_max=0.0)),
    ("circle/no_traj+no_sim", (), lambda c: c.circle(start=False)),
    # ---- mpcq_replace_trajectories
    ("replace/null", T, lambda c: c.replace(null=True)),
    ("replace/no_traj", (), lambda c: c.replace()),
    ("replace/count_neg", T, lambda c: c.replace(count=-1)),
    ("replace/count_B+1", T, lambda c: c.replace(count=B + 1)),
    ("replace/index_out_of_range", T, lambda c: c.replace(idx=(0, B), lens=(TMAX, TMAX))),
    ("replace/duplicate", T, lambda c: c.replace(idx=(1, 1), lens=(TMAX, TMAX))),
    ("replace/len_0", T, lambda c: c.replace(lens=(0,))),
    ("replace/len_Tmax+1", T, lambda c: c.replace(lens=(TMAX + 1,))),
    ("replace/null+no_traj", (), lambda c: c.replace(null=True)),
    ("replace/no_traj+count_neg", (), lambda c: c.replace(count=-1)),
    ("replace/index+len_same_row", T, lambda c: c.replace(idx=(B,), lens=(0,))),
    ("replace/len_row0+index_row1", T, lambda c: c.replace(idx=(0, B), lens=(0, TMAX))),
    # ---- mpcq_mission_set
    ("mission_set/null_wp", T, lambda c: c.mission_set(wp=False)),
    ("mission_set/n_wp_0", T, lambda c: c.mission_set(n_wp=0)),
    ("mission_set/n_wp_8", T, lambda c: c.mission_set(n_wp=8)),
    ("mission_set/L_0", T, lambda c: c.mission_set(L=0)),
    ("mission_set/nonlinear_2", T, lambda c: c.mission_set(nonlinear=2)),
    ("mission_set/v_max_0", T, lambda c: c.mission_set(v=0.0)),
    ("mission_set/dt_inf", T, lambda c: c.mission_set(dt=INF)),
    ("mission_set/order_1", T, lambda c: c.mission_set(order=1)),
    ("mission_set/bad_opts", T, lambda c: c.mission_set(nonlinear=1, opts=c.opts(**BAD_OPTS))),
    ("mission_set/queue_too_large", T, lambda c: c.mission_set(L=1 << 30)),
    ("mission_set/leg0_neg", T, lambda c: c.mission_set(leg0=[0, -1, 0])),
    ("mission_set/leg0_L+1", T, lambda c: c.mission_set(leg0=[0, 0, 2])),
    ("mission_set/no_traj", (), lambda c: c.mission_set()),
    ("mission_set/null_wp+n_wp_0", T, lambda c: c.mission_set(wp=False, n_wp=0)),
    ("mission_set/n_wp_0+L_0", T, lambda c: c.mission_set(n_wp=0, L=0)),
    ("mission_set/L_0+nonlinear_2", T, lambda c: c.mission_set(L=0, nonlinear=2)),
    ("mission_set/nonlinear_2+v_max_0", T, lambda c: c.mission_set(nonlinear=2, v=0.0)),
    ("mission_set/v_max_0+order_1", T, lambda c: c.mission_set(v=0.0, order=1)),
    ("mission_set/order_1+bad_opts", T, lambda c: c.mission_set(order=1, nonlinear=1, opts=c.opts(**BAD_OPTS))),
    ("mission_set/bad_opts+queue_too_large", T, lambda c: c.mission_set(L=1 << 30, nonlinear=1, opts=c.opts(**BAD_OPTS))),
    ("mission_set/bad_opts+leg0_neg", T, lambda c: c.mission_set(nonlinear=1, opts=c.opts(**BAD_OPTS), leg0=[-1, 0, 0])),
    ("mission_set/leg0_neg+no_traj", (), lambda c: c.mission_set(leg0=[-1, 0, 0])),
    ("mission_set/linear_ignores_bad_opts", T, lambda c: c.mission_set(opts=c.opts(**BAD_OPTS))),
    # ---- mpcq_mission_set_legs
    ("set_legs/null_legs", T, lambda c: c.set_legs(legs=None)),
    ("set_legs/L_0", T, lambda c: c.set_legs(L=0)),
    ("set_legs/n_wp_0_with_wp", T, lambda c: c.set_legs(wp=True, n_wp=0)),
    ("set_legs/n_wp_8_with_wp", T, lambda c: c.set_legs(wp=True, n_wp=8)),
    ("set_legs/without_wp_ignores_n_wp_8", T, lambda c: c.set_legs(n_wp=8)),
    ("set_legs/nonlinear_2", T, lambda c: c.set_legs(nonlinear=2)),
    ("set_legs/dt_0", T, lambda c: c.set_legs(dt=0.0)),
    ("set_legs/order_5", T, lambda c: c.set_legs(order=5)),
    ("set_legs/bad_opts", T, lambda c: c.set_legs(nonlinear=1, opts=c.opts(**BAD_OPTS))),
    ("set_legs/queue_too_large", T, lambda c: c.set_legs(legs=c.legs(), L=1 << 30)),
    ("set_legs/unknown_kind", T, lambda c: c.set_legs(legs=c.legs(kind=(1, 0, 5)))),
    ("set_legs/reserved", T, lambda c: c.set_legs(legs=c.legs(reserved=(0, 0, 1)))),
    ("set_legs/waypoint_leg_without_wp", T, lambda c: c.set_legs(legs=c.legs(kind=(2, 0, 0)))),
    ("set_legs/leg_v_max_0", T, lambda c: c.set_legs(legs=c.legs(v_max=(0, 0, 0.0)))),
    ("set_legs/leg_a_max_inf", T, lambda c: c.set_legs(legs=c.legs(a_max=(1, 0, INF)))),
    ("set_legs/circle_radius_0", T, lambda c: c.set_legs(legs=c.legs(radius=(2, 0, 0.0)))),
    ("set_legs/leg0_L+1", T, lambda c: c.set_legs(leg0=[2, 0, 0])),
    ("set_legs/no_traj", (), lambda c: c.set_legs()),
    ("set_legs/null_legs+L_0", T, lambda c: c.set_legs(legs=None, L=0)),
    ("set_legs/L_0+n_wp_0", T, lambda c: c.set_legs(wp=True, L=0, n_wp=0)),
    ("set_legs/n_wp_8+nonlinear_2", T, lambda c: c.set_legs(wp=True, n_wp=8, nonlinear=2)),
    ("set_legs/nonlinear_2+dt_0", T, lambda c: c.set_legs(nonlinear=2, dt=0.0)),
    ("set_legs/dt_0+order_5", T, lambda c: c.set_legs(dt=0.0, order=5)),
    ("set_legs/order_5+bad_opts", T, lambda c: c.set_legs(order=5, nonlinear=1, opts=c.opts(**BAD_OPTS))),
    ("set_legs/bad_opts+unknown_kind", T, lambda c: c.set_legs(legs=c.legs(kind=(0, 0, 5)), nonlinear=1, opts=c.opts(**BAD_OPTS))),
    ("set_legs/reserved_leg0+unknown_kind_leg1", T, lambda c: c.set_legs(legs=c.legs(reserved=(0, 0, 1), kind=(1, 0, 5)))),
    ("set_legs/unknown_kind+reserved_same_leg", T, lambda c: c.set_legs(legs=c.legs(reserved=(1, 0, 1), kind=(1, 0, 5)))),
    ("set_legs/leg_v_max_0+leg0", T, lambda c: c.set_legs(legs=c.legs(v_max=(0, 0, 0.0)), leg0=[2, 0, 0])),
    ("set_legs/leg0+no_traj", (), lambda c: c.set_legs(leg0=[2, 0, 0])),
    # ---- mpcq_mission_get / _stop
    ("mission_get/no_mission", T, lambda c: c.lib.mpcq_mission_get(c.h, None, None, None, None, None, None)),
    ("mission_stop/no_mission", T, lambda c: c.lib.mpcq_mission_stop(c.h)),
    # ---- mpcq_explore_*
    ("explore_start/no_mission", T, lambda c: c.explore()),
    ("explore_start/null_rules", T + ("mission",), lambda c: c.explore(rules=None)),
    ("explore_start/rule_size", T + ("mission",), lambda c: c.explore(size=EXPLORE_RULE_DTYPE.itemsize + 8)),
    ("explore_start/env_without_samples", T + ("mission",), lambda c: c.explore(env=True)),
    ("explore_start/samples_without_env", T + ("mission",), lambda c: c.explore(samples=[1, 1, 1])),
    ("explore_start/step_0", T + ("mission",), lambda c: c.explore(rules=c.rules(step=(1, 0.0)))),
    ("explore_start/desired_nan", T + ("mission",), lambda c: c.explore(rules=c.rules(desired=(0, NAN)))),
    ("explore_start/v_limit_inf", T + ("mission",), lambda c: c.explore(rules=c.rules(v_limit=(2, INF)))),
    ("explore_start/a_limit_neg", T + ("mission",), lambda c: c.explore(rules=c.rules(a_limit=(0, -1.0)))),
    ("explore_start/mode_2", T + ("mission",), lambda c: c.explore(rules=c.rules(mode=(1, 2)))),
    ("explore_start/axes_0", T + ("mission",), lambda c: c.explore(rules=c.rules(axes=(0, 0)))),
    ("explore_start/axes_8", T + ("mission",), lambda c: c.explore(rules=c.rules(axes=(2, 8)))),
    ("explore_start/samples0_neg", T + ("mission",), lambda c: c.explore(env=True, samples=[1, -1, 1])),
    ("explore_start/no_mission+null_rules", T, lambda c: c.explore(rules=None)),
    ("explore_start/null_rules+rule_size", T + ("mission",), lambda c: c.explore(rules=None, size=1)),
    ("explore_start/rule_size+env_without_samples", T + ("mission",), lambda c: c.explore(size=1, env=True)),
    ("explore_start/env_without_samples+step_0", T + ("mission",), lambda c: c.explore(rules=c.rules(step=(0, 0.0)), env=True)),
    ("explore_start/mode_quad0+step_quad1", T + ("mission",), lambda c: c.explore(rules=c.rules(mode=(0, 2), step=(1, 0.0)))),
    ("explore_start/step+mode_same_quad", T + ("mission",), lambda c: c.explore(rules=c.rules(mode=(1, 2), step=(1, 0.0)))),
    ("explore_start/axes+samples0_same_quad", T + ("mission",), lambda c: c.explore(rules=c.rules(axes=(1, 0)), env=True, samples=[1, -1, 1])),
    ("explore_get/not_running", T + ("mission",), lambda c: c.lib.mpcq_explore_get(c.h, None, None, None)),
    ("explore_stop/not_running", T + ("mission",), lambda c: c.lib.mpcq_explore_stop(c.h)),
    ("explore_get/after_mission_stop", T + ("mission", "explore"), lambda c: c.lib.mpcq_mission_stop(c.h) or c.lib.mpcq_explore_get(c.h, None, None, None)),
    ("explore_stop/after_mission_set", T + ("mission", "explore"), lambda c: c.setup_mission() or c.lib.mpcq_explore_stop(c.h)),
    # ---- mpcq_record_*
    ("record_start/active", ("rec_x",), lambda c: c.record_start()),
    ("record_start/count_0_with_quads", (), lambda c: c.record_start(quads=[0], count=0)),
    ("record_start/fields_0", (), lambda c: c.record_start(fields=0)),
    ("record_start/fields_unknown_bit", (), lambda c: c.record_start(fields=512 | REC_X)),
    ("record_start/every_0", (), lambda c: c.record_start(every=0)),
    ("record_start/capacity_0", (), lambda c: c.record_start(capacity=0)),
    ("record_start/rgp_fields_nb0", ("nb0",), lambda c: c.record_start(fields=REC_MU)),
    ("record_start/index_out_of_range", (), lambda c: c.record_start(quads=[0, B], count=2)),
    ("record_start/index_neg", (), lambda c: c.record_start(quads=[-1], count=1)),
    ("record_start/duplicate", (), lambda c: c.record_start(quads=[2, 2], count=2)),
    ("record_start/active+fields_0", ("rec_x",), lambda c: c.record_start(fields=0)),
    ("record_start/count_0+fields_0", (), lambda c: c.record_start(quads=[0], count=0, fields=0)),
    ("record_start/fields_0+every_0", (), lambda c: c.record_start(fields=0, every=0)),
    ("record_start/every_0+rgp_fields_nb0", ("nb0",), lambda c: c.record_start(fields=REC_MU, every=0)),
    ("record_start/rgp_fields_nb0+duplicate", ("nb0",), lambda c: c.record_start(quads=[1, 1], count=2, fields=REC_C)),
    ("record_info/none", (), lambda c: c.lib.mpcq_record_info(c.h, None, None, None)),
    ("record_get/none", (), lambda c: c.lib.mpcq_record_get(c.h, REC_X, c.d(B, 4, 13))),
    ("record_get/field_0", ("rec_x",), lambda c: c.lib.mpcq_record_get(c.h, 0, c.d(B, 4, 13))),
    ("record_get/two_fields", ("rec",), lambda c: c.lib.mpcq_record_get(c.h, 3, c.d(B, 4, 13))),
    ("record_get/not_recorded", ("rec_x",), lambda c: c.lib.mpcq_record_get(c.h, 2, c.d(B, 4, 13))),
    ("record_get/solver_field", ("rec",), lambda c: c.lib.mpcq_record_get(c.h, REC_SOLVER, c.d(B, 4, 13))),
    ("record_get/null_out", ("rec_x",), lambda c: c.lib.mpcq_record_get(c.h, REC_X, None)),
    ("record_get/none+field_0", (), lambda c: c.lib.mpcq_record_get(c.h, 0, None)),
    ("record_get/not_recorded+null_out", ("rec_x",), lambda c: c.lib.mpcq_record_get(c.h, 2, None)),
    ("record_get_solver/none", (), lambda c: c.lib.mpcq_record_get_solver(c.h, None)),
    ("record_get_solver/not_recorded", ("rec_x",), lambda c: c.lib.mpcq_record_get_solver(c.h, c.i([0] * 64))),
    ("record_get_solver/null_out", ("rec",), lambda c: c.lib.mpcq_record_get_solver(c.h, None)),
    ("record_get_solver/not_recorded+null_out", ("rec_x",), lambda c: c.lib.mpcq_record_get_solver(c.h, None)),
    ("record_get_periods/none", (), lambda c: c.lib.mpcq_record_get_periods(c.h, None)),
    ("record_get_periods/null_out", ("rec_x",), lambda c: c.lib.mpcq_record_get_periods(c.h, None)),
    ("record_clear/none", (), lambda c: c.lib.mpcq_record_clear(c.h)),
    ("record_stop/none", (), lambda c: c.lib.mpcq_record_stop(c.h)),
    # ---- mpcq_record_predict
    ("record_predict/none", (), lambda c: c.record_predict()),
    ("record_predict/null_xq", ("rec",), lambda c: c.record_predict(xq=False)),
    ("record_predict/no_output", ("rec",), lambda c: c.record_predict(mean=False)),
    ("record_predict/M_0", ("rec",), lambda c: c.record_predict(M=0)),
    ("record_predict/M_4097", ("rec",), lambda c: c.record_predict(M=4097)),
    ("record_predict/nb0", ("nb0", "rec_x"), lambda c: c.record_predict()),
    ("record_predict/mu_not_recorded", ("rec_x",), lambda c: c.record_predict()),
    ("record_predict/var_needs_C", ("rec_mu",), lambda c: c.record_predict(var=True)),
    ("record_predict/row_window_empty", ("rec",), lambda c: c.record_predict()),
    ("record_predict/row0_neg", ("rec",), lambda c: c.record_predict(row0=-1)),
    ("record_predict/none+null_xq", (), lambda c: c.record_predict(xq=False)),
    ("record_predict/null_xq+no_output", ("rec",), lambda c: c.record_predict(xq=False, mean=False)),
    ("record_predict/no_output+M_0", ("rec",), lambda c: c.record_predict(mean=False, M=0)),
    ("record_predict/M_0+nb0", ("nb0", "rec_x"), lambda c: c.record_predict(M=0)),
    ("record_predict/M_0+mu_not_recorded", ("rec_x",), lambda c: c.record_predict(M=0)),
    ("record_predict/mu_not_recorded+row0_neg", ("rec_x",), lambda c: c.record_predict(row0=-1)),
    ("record_predict/var_needs_C+row0_neg", ("rec_mu",), lambda c: c.record_predict(var=True, row0=-1)),
    # ---- mpcq_rgp_predict
    ("rgp_predict/per_quad_2", (), lambda c: c.rgp_predict(per_quad=2)),
    ("rgp_predict/null_xq", (), lambda c: c.rgp_predict(xq=False)),
    ("rgp_predict/no_output", (), lambda c: c.rgp_predict(mean=False)),
    ("rgp_predict/M_0", (), lambda c: c.rgp_predict(M=0)),
    ("rgp_predict/M_4097", (), lambda c: c.rgp_predict(M=4097)),
    ("rgp_predict/nb0", ("nb0",), lambda c: c.rgp_predict()),
    ("rgp_predict/per_quad_2+null_xq", (), lambda c: c.rgp_predict(per_quad=2, xq=False)),
    ("rgp_predict/null_xq+M_0", (), lambda c: c.rgp_predict(xq=False, M=0)),
    ("rgp_predict/M_0+nb0", ("nb0",), lambda c: c.rgp_predict(M=0)),
    # ---- mpcq_rgp_train / mpcq_record_train
    ("rgp_train/null_spec", (), lambda c: c.rgp_train(spec=None)),
    ("rgp_train/null_out", (), lambda c: c.rgp_train(out=None)),
    ("rgp_train/every_output_null", (), lambda c: c.rgp_train(out=c.out(mu=False))),
    ("rgp_train/mode_0", (), lambda c: c.rgp_train(spec=c.spec(mode=0))),
    ("rgp_train/pair_next_2", (), lambda c: c.rgp_train(spec=c.spec(pair_next=2))),
    ("rgp_train/nb_neg", (), lambda c: c.rgp_train(spec=c.spec(nb=-1))),
    ("rgp_train/nb_65", (), lambda c: c.rgp_train(spec=c.spec(nb=65, basis=True, theta=1.0))),
    ("rgp_train/nb_without_basis", (), lambda c: c.rgp_train(spec=c.spec(nb=3))),
    ("rgp_train/nb_0_with_basis", (), lambda c: c.rgp_train(spec=c.spec(basis=True))),
    ("rgp_train/regress_with_mu_eta", (), lambda c: c.rgp_train(out=c.out(mu_eta=True))),
    ("rgp_train/length_scale_0", (), lambda c: c.rgp_train(spec=c.spec(nb=3, basis=True, theta=0.0))),
    ("rgp_train/nb0", ("nb0",), lambda c: c.rgp_train()),
    ("rgp_train/null_samples", (), lambda c: c.rgp_train(samples=False)),
    ("rgp_train/S_0", (), lambda c: c.rgp_train(S=0)),
    ("rgp_train/T_0", (), lambda c: c.rgp_train(T=0)),
    ("rgp_train/T_1_pair_next", (), lambda c: c.rgp_train(spec=c.spec(pair_next=1), T=1)),
    ("rgp_train/every_output_null+mode_0", (), lambda c: c.rgp_train(spec=c.spec(mode=0), out=c.out(mu=False))),
    ("rgp_train/mode_0+pair_next_2", (), lambda c: c.rgp_train(spec=c.spec(mode=0, pair_next=2))),
    ("rgp_train/regress_with_mu_eta+length_scale_0", (), lambda c: c.rgp_train(spec=c.spec(nb=3, basis=True, theta=0.0), out=c.out(mu_eta=True))),
    ("rgp_train/nb0+null_samples", ("nb0",), lambda c: c.rgp_train(samples=False)),
    ("rgp_train/null_samples+S_0", (), lambda c: c.rgp_train(samples=False, S=0)),
    ("rgp_train/S_0+T_0", (), lambda c: c.rgp_train(S=0, T=0)),
    ("record_train/none", (), lambda c: c.record_train()),
    ("record_train/null_spec", ("rec",), lambda c: c.record_train(spec=None)),
    ("record_train/mode_3", ("rec",), lambda c: c.record_train(spec=c.spec(mode=3))),
    ("record_train/nb0", ("nb0", "rec_x"), lambda c: c.record_train()),
    ("record_train/drag_not_recorded", ("rec_x",), lambda c: c.record_train()),
    ("record_train/row_window_empty", ("rec",), lambda c: c.record_train()),
    ("record_train/none+null_spec", (), lambda c: c.record_train(spec=None)),
    ("record_train/mode_3+drag_not_recorded", ("rec_x",), lambda c: c.record_train(spec=c.spec(mode=3))),
    ("record_train/drag_not_recorded+row0_neg", ("rec_x",), lambda c: c.record_train(row0=-1)),
    # ---- mpcq_score_*
    ("score_start/flights_0", T, lambda c: c.lib.mpcq_score_start(c.h, 0, 0)),
    ("score_start/tail_rows_neg", T, lambda c: c.lib.mpcq_score_start(c.h, 1, -1)),
    ("score_start/table_too_large", T, lambda c: c.lib.mpcq_score_start(c.h, 1 << 27, 0)),
    ("score_start/no_traj", (), lambda c: c.lib.mpcq_score_start(c.h, 1, 0)),
    ("score_start/flights_0+no_traj", (), lambda c: c.lib.mpcq_score_start(c.h, 0, 0)),
    ("score_start/table_too_large+no_traj", (), lambda c: c.lib.mpcq_score_start(c.h, 1 << 27, 0)),
    ("score_get/not_running", T, lambda c: c.lib.mpcq_score_get(c.h, None, None, None, None)),
    ("score_clear/not_running", T, lambda c: c.lib.mpcq_score_clear(c.h)),
    ("score_stop/not_running", T, lambda c: c.lib.mpcq_score_stop(c.h)),
    # ---- mpcq_fleet_*
    ("fleet_set/null", (), lambda c: c.fleet_set(plants=None)),
    ("fleet_set/plant_size", (), lambda c: c.fleet_set(size=PLANT_DTYPE.itemsize - 8)),
    ("fleet_set/period0_-2", (), lambda c: c.fleet_set(period0=-2)),
    ("fleet_set/mass_0", (), lambda c: c.fleet_set(plants=c.plants(mass=(1, None, 0.0)))),
    ("fleet_set/J_nan", (), lambda c: c.fleet_set(plants=c.plants(J=(0, 1, NAN)))),
    ("fleet_set/x_f_inf", (), lambda c: c.fleet_set(plants=c.plants(x_f=(2, 3, INF)))),
    ("fleet_set/rotor_functionality_1.5", (), lambda c: c.fleet_set(plants=c.plants(rotor_functionality=(0, 2, 1.5)))),
    ("fleet_set/payload_nan", (), lambda c: c.fleet_set(plants=c.plants(payload_mass=(1, None, NAN)))),
    ("fleet_set/null+plant_size", (), lambda c: c.fleet_set(plants=None, size=1)),
    ("fleet_set/plant_size+period0", (), lambda c: c.fleet_set(size=1, period0=-2)),
    ("fleet_set/period0+mass_0", (), lambda c: c.fleet_set(plants=c.plants(mass=(0, None, 0.0)), period0=-2)),
    ("fleet_set/J_quad0+mass_quad1", (), lambda c: c.fleet_set(plants=c.plants(J=(0, 2, -1.0), mass=(1, None, 0.0)))),
    ("fleet_set/mass+J_same_quad", (), lambda c: c.fleet_set(plants=c.plants(J=(1, 0, -1.0), mass=(1, None, NAN)))),
    ("fleet_get/none", (), lambda c: c.lib.mpcq_fleet_get(c.h, None, PLANT_DTYPE.itemsize, None)),
    ("fleet_get/plant_size", ("fleet",), lambda c: c.lib.mpcq_fleet_get(c.h, None, 1, None)),
    ("fleet_get/none+plant_size", (), lambda c: c.lib.mpcq_fleet_get(c.h, None, 1, None)),
    ("fleet_stop/none", (), lambda c: c.lib.mpcq_fleet_stop(c.h)),
]


def run_cases(lib_path, ids=None):
    """{id: {"rc": return code, "error": mpcq_last_error() (or "" when rc == 0)}} of the cases (ids: a subset)."""
    out = {}
    for cid, state, call in CASES:
        if ids is not None and cid not in ids:
            continue
        c = Ctx(lib_path, state)
        try:
            rc = int(call(c))
            out[cid] = dict(rc=rc, error=c.lib.mpcq_last_error().decode() if rc else "")
        finally:
            c.e.close()
    return out

"""The nonlinear stage of the min-snap generator: the objective and the Subplex optimiser of the host library (mpcq_minsnap_nl_objective,
mpcq_minsnap_nonlinear), and the device generator mpcq_replan_nonlinear on the lane emulator (CPU, small batches) and on the MI355X
(-m gpu).  The yardstick of the device is the host library (bit for bit); the yardstick of the closed loop is the fp64 CPU oracle."""
import os
import subprocess

import numpy as np
import pytest

from parity_cases import rel_err, rel_err_per_instance
from mpc_quad_ros_amd import _lib
from mpc_quad_ros_amd.engine import REPLAN_BAD_INPUT, REPLAN_DONE, REPLAN_LIMITS, REPLAN_SKIPPED, REPLAN_TOO_LONG, Engine
from mpc_quad_ros_amd.params import EngineConfig, hummingbird, rgp_basis_linspace
from mpc_quad_ros_amd import trajectories as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "wave_emu")
EMU = os.path.join(EMU_DIR, "libmpcq_emu.so")
HOVER = np.array([0, 0, 3.0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0])
MPCQ_ERR_INVALID, MPCQ_ERR_STATE = -1, -3
# the reference's static waypoint file (tests/test_minsnap.py STATIC_WAYPOINTS) and its logged flights
STATIC_WAYPOINTS = np.array([[0, 0, 3.0], [5, 0, 6], [5, 5, 9], [-5, 5, 12], [-5, -5, 9], [5, -5, 6], [0, 0, 3]])
LOGGED = (((10.0, 10.0), 12.10), ((15.0, 5.0), 16.30), ((12.0, 12.0), 11.33))
W_T, W_S, CAP = 500.0, 100.0, 1e12
TIGHT = dict(f_rel=0.0, x_rel=0.0)


# ------------------------------------------------------------------ numpy restatement of the objective
def sampled_peaks(pieces):
    """Peak speed / acceleration at the sample points of the generators' limit check: max(2, ceil(T / 0.01)) intervals per segment."""
    vm = am = 0.0
    for P in pieces:
        T = P[0]
        steps = max(2, int(np.ceil(T / 0.01)))
        t = T * np.arange(steps + 1) / steps
        c = P[1:25].reshape(3, 8)
        v, a = np.zeros((3, len(t))), np.zeros((3, len(t)))
        for ax in range(3):                                   # Horner, highest power first (the peaks enter exp(100 (.)))
            for i in range(7, 0, -1):
                v[ax] = v[ax] * t + i * c[ax, i]
            for i in range(7, 1, -1):
                a[ax] = a[ax] * t + float(i * (i - 1)) * c[ax, i]
        vm, am = max(vm, np.linalg.norm(v, axis=0).max()), max(am, np.linalg.norm(a, axis=0).max())
    return vm, am


def closed_form_pieces(wp, T, d):
    """Coefficients c = A(T)^-1 [p v a j](0), [p v a j](T) with A(T)^-1_ia = A(1)^-1_ia T^(r_a - i): the form the objective evaluates.
    (The soft terms amplify a peak's relative error by w_s vpk / v_max ~ 100, so they are compared on pieces of this form.)"""
    A = np.zeros((8, 8))
    for r in range(4):
        for i in range(8):
            f = float(np.prod([i - k for k in range(r)])) if i >= r else 0.0
            A[r, i] = f if i == r else 0.0
            A[4 + r, i] = f
    Ai = np.linalg.inv(A)
    n = len(wp)
    pieces = np.zeros((n - 1, 33))
    for s in range(n - 1):
        pieces[s, 0] = T[s]
        for ax in range(3):
            dv = np.zeros(8)
            for a in range(8):
                v, r = s + a // 4, a % 4
                dv[a] = wp[v, ax] if r == 0 else (0.0 if v in (0, n - 1) else d[v - 1, ax, r - 1])
            pieces[s, 1 + 8 * ax:9 + 8 * ax] = [(Ai[i] * T[s] ** (np.arange(8) % 4 - i) * dv).sum() for i in range(8)]
    return pieces


def numpy_objective(wp, T, d, v_max, a_max, order, w_t=W_T, w_s=W_S, cap=CAP, time_cost=2, soft=1):
    _, J = tr.minsnap_from_derivatives(wp, T, d, order)
    pieces = closed_form_pieces(wp, T, d)
    tc = w_t * T.sum() ** 2 if time_cost == 2 else w_t * T.sum()
    vm, am = sampled_peaks(pieces)
    with np.errstate(over="ignore"):
        sv = min(cap, np.exp(w_s * (vm / v_max - 1))) if soft else 0.0
        sa = min(cap, np.exp(w_s * (am / a_max - 1))) if soft else 0.0
    return np.array([J, tc, sv, sa])


def random_flight(rng, n_wp, size=5.0):
    return np.vstack([rng.uniform(-size, size, 3) + [0, 0, 7.5], rng.uniform(-size, size, (n_wp, 3)) + [0, 0, 7.5]])


def test_objective_matches_numpy_restatement():
    rng = np.random.default_rng(0)
    checked_cap = False
    for trial in range(24):
        n = 2 + trial % 6
        wp = random_flight(rng, n - 1)
        order = 2 + trial % 3
        v_max, a_max = rng.uniform(3, 15), rng.uniform(3, 15)
        T = rng.uniform(0.3, 4.0, n - 1)
        d = rng.uniform(-1, 1, (n - 2, 3, 3)) * [2.0, 2.0, 4.0]
        kw = [dict(), dict(time_cost=1, time_penalty=37.0), dict(use_soft_constraints=0), dict(soft_constraint_cap=50.0, soft_constraint_weight=7.0)][trial % 4]
        f, parts = tr.minsnap_nl_objective(wp, T, d, v_max, a_max, order, kw or None)
        ref = numpy_objective(wp, T, d, v_max, a_max, order, w_t=kw.get("time_penalty", W_T), w_s=kw.get("soft_constraint_weight", W_S),
                              cap=kw.get("soft_constraint_cap", CAP), time_cost=kw.get("time_cost", 2), soft=kw.get("use_soft_constraints", 1))
        # the soft terms: 1e-12 relative times their condition number w_s vpk / v_max (exp(w_s (r - 1)) amplifies an error of r)
        vm, am = sampled_peaks(closed_form_pieces(wp, T, d))
        w_s = kw.get("soft_constraint_weight", W_S)
        # the derivative cost: the objective's closed form (A(1)^-1 scaled by powers of T) against mpcq_minsnap_from_derivatives' elimination
        # at T -- two evaluations of an ill-conditioned quadratic form, which agree to ~1e-11
        cond = [10.0, 1.0, max(1.0, w_s * vm / v_max), max(1.0, w_s * am / a_max)]
        for k in range(4):
            assert abs(parts[k] - ref[k]) <= 1e-12 * cond[k] * abs(ref[k]) or parts[k] == ref[k], (trial, k, parts[k], ref[k])
        assert f == ((parts[0] + parts[1]) + parts[2]) + parts[3]
        checked_cap = checked_cap or (kw.get("soft_constraint_cap") == 50.0 and parts[2:].max() == 50.0)
        if kw.get("use_soft_constraints") == 0:
            assert parts[2] == 0 and parts[3] == 0
    assert checked_cap
    with pytest.raises(ValueError):
        tr.minsnap_nl_objective(STATIC_WAYPOINTS[:3], [1.0, -1.0], np.zeros((1, 3, 3)), 10, 10)
    with pytest.raises(ValueError):
        tr.minsnap_nl_objective(STATIC_WAYPOINTS[:3], [1.0, 1.0], np.zeros((1, 3, 3)), 10, 10, 3, dict(time_cost=3))


@pytest.mark.parametrize("order", [2, 3, 4])
def test_single_segment_analytic_optimum(order):
    """One segment, soft limits off: f = C T^-(2r-1) + w_t T^2, minimised at T* = ((2r-1) C / (2 w_t))^(1/(2r+1))."""
    wp = np.array([[0, 0, 3.0], [40.0, -25.0, 9.0]])
    _, C = tr.minsnap_from_derivatives(wp, np.array([1.0]), np.zeros((0, 3, 3)), order)
    r = order
    Tstar = ((2 * r - 1) * C / (2 * W_T)) ** (1 / (2 * r + 1))
    assert Tstar > 1.0
    # (f_rel 0 rather than 1e-10: near T* a relative f change of 1e-10 still allows a relative T error of ~5e-6 for order 4)
    pieces, _, info = tr.minsnap_pieces_nonlinear(wp, 10.0, 10.0, order, dict(use_soft_constraints=0, f_rel=0.0, x_rel=1e-10, max_evaluations=5000))
    assert abs(pieces[0, 0] / Tstar - 1) < 1e-6, (pieces[0, 0], Tstar, info)


def grad(fun, x, rel=1e-6):
    g = np.zeros_like(x)
    for i in range(len(x)):
        h = rel * max(abs(x[i]), 1.0)
        e = np.zeros_like(x)
        e[i] = h
        g[i] = (fun(x + e) - fun(x - e)) / (2 * h)
    return g


def test_stationary_point_without_tolerances():
    wp = np.array([[0, 0, 3.0], [6, 1, 5], [4, 7, 8], [-3, 4, 6]])
    v_max, a_max, order = 30.0, 30.0, 3                  # (limits wide enough that no bound of the box is active at the optimum)
    opts = dict(use_soft_constraints=0, max_evaluations=20000, **TIGHT)
    m = len(wp) - 1

    def f(x):
        return tr.minsnap_nl_objective(wp, x[:m], x[m:].reshape(-1, 3, 3), v_max, a_max, order, opts)[0]
    _, d0, info0 = tr.minsnap_pieces_nonlinear(wp, v_max, a_max, order, dict(opts, max_evaluations=1))
    pieces, d, info = tr.minsnap_pieces_nonlinear(wp, v_max, a_max, order, opts)
    x0 = np.concatenate([np.maximum(tr.minsnap_estimate_times(wp, v_max, a_max), 0.1), d0.reshape(-1)])
    x1 = np.concatenate([pieces[:, 0], d.reshape(-1)])
    assert len(x1) == 21 and info[1] < info[0]
    g0, g1 = np.linalg.norm(grad(f, x0)), np.linalg.norm(grad(f, x1))
    print(f"\ngradient norm {g0:.3e} -> {g1:.3e} ({info[2]:.0f} evaluations)")
    assert g1 <= 1e-3 * g0


def test_optimiser_contract_at_defaults():
    rng = np.random.default_rng(7)
    for trial in range(14):
        n_wp = 1 + trial % 7
        wp = random_flight(rng, n_wp)
        v_max, a_max, order = [(10.0, 10.0, 3), (15.0, 5.0, 3), (12.0, 12.0, 4), (8.0, 6.0, 2)][trial % 4]
        pieces, d, info = tr.minsnap_pieces_nonlinear(wp, v_max, a_max, order)
        assert info[1] <= info[0] and 1 <= info[2] <= 1000
        assert (pieces[:, 0] >= 0.1).all()
        if n_wp > 1:
            assert (np.abs(d[:, :, 0]) <= v_max).all() and (np.abs(d[:, :, 1]) <= a_max).all()
        p2, d2, i2 = tr.minsnap_pieces_nonlinear(wp, v_max, a_max, order)
        assert np.array_equal(pieces, p2) and np.array_equal(d, d2) and np.array_equal(info, i2)
        ref, _ = tr.minsnap_from_derivatives(wp, pieces[:, 0], d, order)
        scale = np.abs(ref[:, 1:25]).max(axis=1, keepdims=True)
        assert np.abs(pieces[:, 1:25] - ref[:, 1:25]).max() <= 1e-9 * scale.max()
        assert info[3] == pieces[:, 0].sum() or abs(info[3] - pieces[:, 0].sum()) < 1e-12 * info[3]
        f, _ = tr.minsnap_nl_objective(wp, pieces[:, 0], d, v_max, a_max, order)
        assert f == info[1]
    small = tr.minsnap_pieces_nonlinear(random_flight(rng, 4), 10, 10, 3, dict(max_evaluations=17))[2]
    assert small[2] == 17
    with pytest.raises(ValueError):
        tr.minsnap_pieces_nonlinear(random_flight(rng, 8), 10, 10, 3)           # 9 vertices: beyond the device limit
    for bad in (dict(max_evaluations=0), dict(f_rel=-1.0), dict(soft_constraint_weight=0.0), dict(use_soft_constraints=2)):
        with pytest.raises(ValueError):
            tr.minsnap_pieces_nonlinear(random_flight(rng, 2), 10, 10, 3, bad)


def test_static_waypoint_file_against_the_logged_flights():
    """The reference's static waypoint file, the three (v_max, a_max) cases of its logs.  At the defaults the optimiser improves on the
    linear stage; run to 30 000 evaluations without tolerances it converges onto shorter flights than the logged ones, which sit at a
    softly penalised acceleration peak (DESIGN.md section 6.1 records the numbers and why the 12 % aim is not met).  That they are a better
    minimum of the same objective, not another objective's optimum: f at the logged flights' own (T, d_P) -- recovered from the logs as in
    tests/test_minsnap.py -- is above f at the converged result."""
    rows = []
    logged_points = logged_T_dP()
    for ((v_max, a_max), logged), (T_log, d_log) in zip(LOGGED, logged_points):
        lin = tr.reference_linear_stage(STATIC_WAYPOINTS, v_max, a_max, 3)
        p0, _, i0 = tr.minsnap_pieces_nonlinear(STATIC_WAYPOINTS, v_max, a_max, 3)
        p1, _, i1 = tr.minsnap_pieces_nonlinear(STATIC_WAYPOINTS, v_max, a_max, 3, dict(max_evaluations=30000, **TIGHT))
        assert i0[1] < i0[0] and i0[3] < lin[:, 0].sum()
        assert i1[1] <= i0[1]
        assert 0.65 < i1[3] / logged < 1.12, (v_max, a_max, i1)
        f_log, _ = tr.minsnap_nl_objective(STATIC_WAYPOINTS, T_log, d_log, v_max, a_max, 3)
        assert abs(T_log.sum() / logged - 1) < 0.01
        assert i1[1] < f_log, (v_max, a_max, i1[1], f_log)
        rows.append((v_max, a_max, logged, lin[:, 0].sum(), i0, i1, f_log))
    print("\nv_max a_max | logged: T f | linear stage | defaults: T vpk apk evals f | 30 000 evals, no tolerances: T vpk apk f")
    for v, a, logged, lin, i0, i1, f_log in rows:
        print(f"{v:5.0f} {a:5.0f} | {logged:6.2f} {f_log:8.0f} | {lin:6.2f} | {i0[3]:6.2f} {i0[4]:5.2f} {i0[5]:5.2f} {i0[2]:5.0f} {i0[1]:8.0f} | "
              f"{i1[3]:6.2f} {i1[4]:5.2f} {i1[5]:5.2f} {i1[1]:8.0f}")


def logged_T_dP():
    """(T, d_P) of the three logged flights through the static waypoint file: the least-squares fit of tests/test_minsnap.py
    (test_logged_references_are_points_of_the_generators_family), which reproduces them to the rounding of the binary's CSV."""
    from scipy.optimize import least_squares
    from test_minsnap import _logged_reference, _piece_boundaries, _sample_exact
    out = []
    for name, dt in (("log_traj0_v10_a10_gp2.npz", 0.1), ("log_traj0_v15_a5_gp2.npz", 0.1), ("log_gazebo_traj0_v12_a12_gp0.npz", 0.01)):
        p, v, t = _logged_reference(name, dt)
        n = len(t)
        idx = _piece_boundaries(t, p, v, STATIC_WAYPOINTS)
        T0 = np.diff(np.array([t[i] if i < n else t[-1] + dt for i in idx]))

        def d_of(P):
            return np.array([[[P[s, 2 + 8 * a], 2 * P[s, 3 + 8 * a], 6 * P[s, 4 + 8 * a]] for a in range(3)] for s in range(1, 6)])

        def res(z):
            if np.any(z[:6] < 0.2):
                return np.full(6 * n, 1e3)
            x = _sample_exact(tr.minsnap_from_derivatives(STATIC_WAYPOINTS, z[:6], z[6:].reshape(5, 3, 3), 3)[0], dt, n)
            return np.concatenate([(x[:, :3] - p).ravel(), (x[:, 3:] - v).ravel()])
        z0 = np.concatenate([T0, d_of(tr.minsnap_solve_order(STATIC_WAYPOINTS, T0, 3)).ravel()])
        sol = least_squares(res, z0, method="lm", xtol=1e-14, ftol=1e-14, gtol=1e-14, max_nfev=3000)
        out.append((sol.x[:6], sol.x[6:].reshape(5, 3, 3)))
    return out


def test_options_struct_and_defaults_have_one_statement():
    """include/mpcq_nl_options.h holds the struct and MPCQ_MINSNAP_NL_DEFAULTS; the ctypes mirror, the host library's defaults and the
    macro agree, and both C ABIs take the struct from that header."""
    import ctypes
    import re
    hdr = open(os.path.join(ROOT, "include", "mpcq_nl_options.h")).read()
    body = re.sub(r"/\*.*?\*/", "", hdr[hdr.index("typedef struct mpcq_minsnap_nl_options {"):hdr.index("} mpcq_minsnap_nl_options;")], flags=re.S)
    names = re.findall(r"\b([a-z_]+)\s*;", body)
    assert names == [f for f, _ in _lib.NlOptions._fields_] and ctypes.sizeof(_lib.NlOptions) == 56
    macro = [float(v) for v in re.search(r"#define MPCQ_MINSNAP_NL_DEFAULTS \{([^}]*)\}", hdr).group(1).split(",")]
    assert macro[:-1] == list(_lib.nl_defaults().values()) and macro[-1] == 0
    assert list(_lib.nl_defaults().values()) == [500.0, 100.0, 1e12, 0.05, 0.1, 1000, 2, 1]
    for h in ("mpcq.h", "mpcq_traj_nl.h"):
        text = open(os.path.join(ROOT, "include", h)).read()
        assert '#include "mpcq_nl_options.h"' in text and "typedef struct mpcq_minsnap_nl_options" not in text, h


def test_segment_times_are_bounded():
    """Every evaluation's work stays finite: time_penalty must be > 0, segment times stay within 10 x their start, a linear stage longer
    than 300 s is refused, and the objective refuses T > 3000 s."""
    import time
    wp = np.array([[0, 0, 3.0], [3.0, 1.0, 4.0]])
    with pytest.raises(ValueError, match=r"\(-1\)"):
        tr.minsnap_pieces_nonlinear(wp, 12.0, 12.0, 3, dict(time_penalty=0.0))
    with pytest.raises(ValueError):
        tr.minsnap_nl_objective(wp, [1.0], np.zeros((0, 3, 3)), 12.0, 12.0, 3, dict(time_penalty=0.0))
    t0 = time.perf_counter()
    pieces, _, info = tr.minsnap_pieces_nonlinear(wp, 12.0, 12.0, 3, dict(time_penalty=1e-9))
    T_start = max(tr.minsnap_estimate_times(wp, 12.0, 12.0)[0], 0.1)
    assert pieces[0, 0] <= 10 * T_start and info[4] > 0 and info[5] > 0
    assert time.perf_counter() - t0 < 5.0
    with pytest.raises(ValueError, match=r"\(-3\)"):
        tr.minsnap_pieces_nonlinear(np.array([[0, 0, 3.0], [20.0, 0, 3.0]]), 0.05, 1.0, 3)   # Nfabian: 800 s
    assert np.isfinite(tr.minsnap_nl_objective(wp, [3000.0], np.zeros((0, 3, 3)), 12.0, 12.0, 3)[0])
    with pytest.raises(ValueError):
        tr.minsnap_nl_objective(wp, [3000.5], np.zeros((0, 3, 3)), 12.0, 12.0, 3)


# ------------------------------------------------------------------ engine cases (lane emulator and MI355X)
@pytest.fixture(scope="module")
def emu():
    subprocess.check_call(["make", "-C", EMU_DIR], stdout=subprocess.DEVNULL)
    return EMU


def config(B, N=10, nb=0, **kw):
    extra = dict(basis=rgp_basis_linspace(12.0, nb), theta=[1.0, 0.1, 0.1]) if nb else {}
    return EngineConfig(batch=B, N=N, T=1.0, quad=hummingbird(), nb=nb, dt_pred=0.01, **extra, **kw)


def hover_slots(B, Tmax, length, x0=None):
    x0 = np.tile(HOVER, (B, 1)) if x0 is None else x0
    traj = np.repeat(x0[:, None, :], Tmax, axis=1).copy()
    traj[:, :, 3:7] = [1, 0, 0, 0]
    traj[:, :, 7:] = 0
    return traj, np.full(B, length, np.int32)


def expect_rc(rc, fn, *args):
    with pytest.raises(_lib.MpcqError, match=f"mpcq error {rc}:"):
        fn(*args)


def case_parity(lib, B, precision=0, seed=0, Tmax=2400, combos=None, host_sample=None, opts=None):
    """Device pieces, d_free and info bit-identical to mpcq_minsnap_nonlinear; sampled slot rows = mpcq_minsnap_sample of the host
    pieces within one quantum of the 6-decimal rounding; padding = the last row.  host_sample: check a seeded subset of that size."""
    e = Engine(config(B, precision=precision), lib_path=lib)
    e.set_trajectories(*hover_slots(B, Tmax, 5))
    rng = np.random.default_rng(seed)
    combos = combos or [(1, 3, (12.0, 12.0)), (3, 3, (15.0, 5.0)), (6, 4, (10.0, 10.0)), (7, 2, (12.0, 12.0))]
    checked = compared = 0
    for n_wp, order, (v, a) in combos:
        start = rng.uniform(-5, 5, (B, 3)) + [0, 0, 7.5]
        wp = rng.uniform(-5, 5, (B, n_wp, 3)) + [0, 0, 7.5]
        codes, info, pieces, d_free = e.replan_nonlinear(wp, v, a, 0.01, order, start=start, mask=np.ones(B), opts=opts, return_pieces=True)
        traj, lens = e.get_trajectories()
        idx = range(B) if host_sample is None else np.sort(rng.choice(B, host_sample, replace=False))
        for b in idx:
            hp, hd, hi = tr.minsnap_pieces_nonlinear(np.vstack([start[b], wp[b]]), v, a, order, opts)
            assert np.array_equal(pieces[b], hp), (n_wp, order, b, np.abs(pieces[b] - hp).max())
            assert np.array_equal(d_free[b], hd) and np.array_equal(info[b], hi), (n_wp, order, b, info[b], hi)
            compared += 1
            x = tr.sample_polynomial_trajectory_native(hp, 0.01)[0]
            if len(x) > Tmax:
                assert codes[b] == REPLAN_TOO_LONG
                continue
            assert codes[b] == REPLAN_DONE and lens[b] == len(x), (codes[b], lens[b], len(x))
            got = traj[b]
            assert np.abs(got[:len(x), [0, 1, 2, 7, 8, 9]] - x[:, [0, 1, 2, 7, 8, 9]]).max() <= 1.5e-6
            assert np.array_equal(got[:len(x), [3, 4, 5, 6, 10, 11, 12]], x[:, [3, 4, 5, 6, 10, 11, 12]])
            assert (got[len(x):] == got[len(x) - 1]).all()
            checked += 1
    st = e.get_state()
    assert (st["idx"] == 0).all() and (e.get_finished() == 0).all()
    e.close()
    return compared, checked


def case_slot_isolation(lib, B, K=3, seed=1):
    e = Engine(config(B, nb=10), lib_path=lib)
    Tmax = 600
    rng = np.random.default_rng(seed)
    x0 = np.tile(HOVER, (B, 1))
    x0[:, 0:3] += rng.uniform(-0.3, 0.3, (B, 3))
    traj, lens = hover_slots(B, Tmax, 3, x0)
    lens[::2] = 200
    e.set_trajectories(traj, lens)
    e.sim_reset(x0)
    e.sim_steps(K, 2, 5e-3)
    traj0, lens0 = e.get_trajectories()
    st0, sv0 = e.get_state(), e.get_solver_state()
    mask = (rng.uniform(size=B) < 0.5).astype(np.int32)
    mask[0], mask[1] = 1, 0
    wp = x0[:, None, 0:3] + rng.uniform(-1, 1, (B, 2, 3))
    wp[mask == 0] = np.nan
    codes, info = e.replan_nonlinear(wp, 12.0, 12.0, mask=mask)
    assert (codes[mask == 0] == REPLAN_SKIPPED).all() and (codes[mask == 1] == REPLAN_DONE).all(), codes
    assert np.isnan(info[mask == 0]).all() and np.isfinite(info[mask == 1]).all()
    traj1, lens1 = e.get_trajectories()
    st1, sv1 = e.get_state(), e.get_solver_state()
    un = mask == 0
    assert np.array_equal(traj1[un], traj0[un]) and np.array_equal(lens1[un], lens0[un])
    assert np.array_equal(st1["idx"][un], st0["idx"][un]) and np.array_equal(sv1["finished"][un], sv0["finished"][un])
    assert (st1["idx"][~un] == 0).all() and (sv1["finished"][~un] == 0).all()
    for k in ("X", "U", "mu", "C", "x_pred_prev", "has_prev"):
        assert np.array_equal(st1[k], st0[k]), k
    for k in ("qp_iter", "stats"):
        assert np.array_equal(sv1[k], sv0[k]), k
    x, _ = e.sim_get_state()                      # start = NULL: the plant's position
    for b in np.flatnonzero(mask)[:3]:
        hp, _, hi = tr.minsnap_pieces_nonlinear(np.vstack([x[b, 0:3], wp[b]]), 12.0, 12.0, 3)
        assert np.array_equal(info[b], hi)
        ref = tr.sample_polynomial_trajectory_native(hp, 0.01)[0]
        assert lens1[b] == len(ref) and np.abs(traj1[b, :len(ref), 0:3] - ref[:, 0:3]).max() <= 1.5e-6
    e.close()


def case_mask_none_picks_finished(lib, B, seed=2):
    e = Engine(config(B), lib_path=lib)
    rng = np.random.default_rng(seed)
    x0 = np.tile(HOVER, (B, 1))
    traj, lens = hover_slots(B, 400, 3, x0)
    lens[rng.uniform(size=B) < 0.4] = 250
    e.set_trajectories(traj, lens)
    e.sim_reset(x0)
    e.sim_steps(4, 2, 5e-3)
    fin = e.get_finished().astype(bool)
    assert fin.any() and not fin.all(), fin
    idx0 = e.get_state()["idx"]
    wp = x0[:, None, 0:3] + rng.uniform(-1, 1, (B, 1, 3))
    codes, info = e.replan_nonlinear(wp, 12.0, 12.0)
    assert (codes[fin] == REPLAN_DONE).all() and (codes[~fin] == REPLAN_SKIPPED).all(), codes
    st = e.get_state()
    assert (e.get_finished() == 0).all()
    assert (st["idx"][fin] == 0).all() and np.array_equal(st["idx"][~fin], idx0[~fin])
    e.close()


def case_errors(lib, B):
    e = Engine(config(B), lib_path=lib)
    wp = np.tile([[0.5, 0.5, 3.5]], (B, 1, 1))
    expect_rc(MPCQ_ERR_STATE, e.replan_nonlinear, wp, 12.0, 12.0)                 # before set_trajectories
    Tmax = 300
    traj, lens = hover_slots(B, Tmax, 10)
    e.set_trajectories(traj, lens)
    expect_rc(MPCQ_ERR_STATE, e.replan_nonlinear, wp, 12.0, 12.0)                 # start = NULL without sim_reset
    start = np.tile(HOVER[:3], (B, 1))
    for kw in (dict(v_max=0.0), dict(a_max=-1.0), dict(dt=0.0), dict(v_max=float("nan")), dict(derivative_to_optimize=1),
               dict(derivative_to_optimize=5), dict(opts=dict(max_evaluations=0)), dict(opts=dict(time_cost=0)),
               dict(opts=dict(soft_constraint_weight=-1.0)), dict(opts=dict(x_rel=float("nan"))), dict(opts=dict(use_soft_constraints=3)),
               dict(opts=dict(time_penalty=0.0))):
        args = dict(wp=wp, v_max=12.0, a_max=12.0, dt=0.01, derivative_to_optimize=3, start=start)
        args.update(kw)
        expect_rc(MPCQ_ERR_INVALID, lambda: e.replan_nonlinear(**args))
    for n_wp in (0, 8):
        bad = np.zeros((B, n_wp, 3)) + [0.5, 0.5, 3.5]
        expect_rc(MPCQ_ERR_INVALID, lambda: e.replan_nonlinear(bad, 12.0, 12.0, start=start))
    rc = e.lib.mpcq_replan_nonlinear(e.h, _lib.d(np.ascontiguousarray(start)), None, 1, 12.0, 12.0, 3, 0.01, None, None, None, None, None, None)
    assert rc == MPCQ_ERR_INVALID
    t0, l0 = e.get_trajectories()
    far = wp.copy()
    far[0, 0] = [20.0, -20.0, 10.0]
    far[1, 0, 2] = np.nan
    far[2, 0] = [2000.0, 0.0, 3.0]                                          # a linear stage of ~330 s: refused before optimising
    codes, info = e.replan_nonlinear(far, 12.0, 12.0, start=start, mask=np.ones(B))
    assert codes[0] == REPLAN_TOO_LONG and codes[1] == REPLAN_BAD_INPUT and codes[2] == REPLAN_LIMITS, codes
    assert (codes[3:] == REPLAN_DONE).all(), codes
    assert np.isfinite(info[0]).all() and np.isnan(info[1:3]).all()         # too long: the flight was planned, not installed
    with pytest.raises(ValueError, match=r"\(-3\)"):
        tr.minsnap_pieces_nonlinear(np.vstack([start[2], far[2]]), 12.0, 12.0, 3)
    t1, l1 = e.get_trajectories()
    assert np.array_equal(t1[:3], t0[:3]) and np.array_equal(l1[:3], l0[:3])
    # info NULL: the same flights
    e.set_trajectories(traj, lens)
    out, ones = np.zeros(B, np.int32), np.ones(B, np.int32)
    assert e.lib.mpcq_replan_nonlinear(e.h, _lib.d(np.ascontiguousarray(start)), _lib.d(np.ascontiguousarray(wp)), 1, 12.0, 12.0, 3, 0.01,
                                       _lib.i(ones), _lib.i(out), None, None, None, None) == 0
    t2, l2 = e.get_trajectories()
    e.set_trajectories(traj, lens)
    codes, info = e.replan_nonlinear(wp, 12.0, 12.0, start=start, mask=np.ones(B))
    t3, l3 = e.get_trajectories()
    assert (out == REPLAN_DONE).all() and (codes == REPLAN_DONE).all()
    assert np.array_equal(t2, t3) and np.array_equal(l2, l3)
    e.close()


def hop_waypoints(x, rng, n_wp=1, size=0.6):
    return x[:, None, 0:3] + rng.uniform(-size, size, (x.shape[0], n_wp, 3))


def case_closed_loop_vs_oracle(lib, B, K, seed=3, nb=10):
    """sim_steps(1), then replan_nonlinear(mask=None), in lockstep with the fp64 oracle fed the engine's plant states and, after every
    replan, the engine's read-back slots."""
    from oracle.oracle import OracleEngine
    cfg = config(B, nb=nb)
    e, o = Engine(cfg, lib_path=lib), OracleEngine(config(B, nb=nb))
    rng = np.random.default_rng(seed)
    x0 = np.tile(HOVER, (B, 1))
    x0[:, 0:3] += rng.uniform(-0.5, 0.5, (B, 3))
    traj, lens = hover_slots(B, 400, 2, x0)
    e.set_trajectories(traj, lens); o.set_trajectories(traj, lens)
    e.sim_reset(x0)
    worst, flights, after = 0.0, 0, []
    for k in range(K):
        x, _ = e.sim_get_state()
        wo, _ = o.step(x)
        e.sim_steps(1, 2, 5e-3)
        _, w = e.sim_get_state()
        dev = max(rel_err_per_instance(w, wo, floor=1e-2), rel_err(w, wo))
        assert dev < 1e-7, (k, dev)
        worst = max(worst, dev)
        x, _ = e.sim_get_state()
        codes, _ = e.replan_nonlinear(hop_waypoints(x, rng), 12.0, 12.0)
        assert ((codes == REPLAN_DONE) | (codes == REPLAN_SKIPPED)).all(), codes
        done = int((codes == REPLAN_DONE).sum())
        if done:
            flights += done
            after.append(k + 1)
            t, ln = e.get_trajectories()
            o.set_trajectories(t, ln)
            o.set_state(idx=e.get_state()["idx"])
    e.close(); o.close()
    return worst, flights, after


def run_continuous(e, rng, K):
    for _ in range(K):
        e.sim_steps(1, 2, 5e-3)
        x, _ = e.sim_get_state()
        e.replan_nonlinear(hop_waypoints(x, rng), 12.0, 12.0)


def snapshot(e):
    x, w = e.sim_get_state()
    t, ln = e.get_trajectories()
    return dict(x=x, w=w, traj=t, len=ln, **{f"st_{k}": v for k, v in e.get_state().items()},
                **{f"sv_{k}": v for k, v in e.get_solver_state().items()})


def case_checkpoint(lib, B, K0=30, K=20, seed=4):
    cfg = config(B, nb=10)
    e = Engine(cfg, lib_path=lib)
    rng = np.random.default_rng(seed)
    x0 = np.tile(HOVER, (B, 1))
    e.set_trajectories(*hover_slots(B, 400, 2, x0))
    e.sim_reset(x0)
    run_continuous(e, rng, K0)
    st, sv, (x, _) = e.get_state(), e.get_solver_state(), e.sim_get_state()
    t, ln = e.get_trajectories()
    assert (ln != 2).any()
    f = Engine(cfg, lib_path=lib)
    f.set_trajectories(t, ln)
    f.set_state(**st)
    f.set_solver_state(**sv)
    f.sim_reset(x)
    state = rng.bit_generator.state
    run_continuous(e, rng, K)
    rng.bit_generator.state = state
    run_continuous(f, rng, K)
    a, b = snapshot(e), snapshot(f)
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), k
    e.close(); f.close()


# ------------------------------------------------------------------ lane emulator (CPU)
def test_emu_parity_with_host(emu):
    compared, installed = case_parity(emu, 2, Tmax=2000)
    assert compared == 8 and installed >= 6


def test_emu_parity_with_host_options(emu):
    opts = dict(time_cost=1, time_penalty=80.0, use_soft_constraints=0, max_evaluations=300, f_rel=0.0, x_rel=0.0)
    case_parity(emu, 2, Tmax=4000, combos=[(4, 3, (10.0, 10.0))], opts=opts)


def test_emu_slot_isolation(emu):
    case_slot_isolation(emu, 4)


def test_emu_mask_none_picks_finished(emu):
    case_mask_none_picks_finished(emu, 6)


def test_emu_errors(emu):
    case_errors(emu, 4)


def test_emu_closed_loop_vs_oracle(emu):
    worst, flights, after = case_closed_loop_vs_oracle(emu, 2, 100)
    print(f"closed loop: worst deviation {worst:.2e}, {flights} flights replanned")
    assert flights >= 2 and any(k < 100 for k in after)


def test_emu_checkpoint_after_replans(emu):
    case_checkpoint(emu, 2, K0=20, K=15)


# ------------------------------------------------------------------ MI355X
gpu = pytest.mark.gpu


@gpu
@pytest.mark.parametrize("precision", [0, 1])
def test_gpu_parity_b8192(precision):
    compared, installed = case_parity(None, 8192, precision=precision, Tmax=1500, combos=[(3, 3, (12.0, 12.0)), (6, 3, (15.0, 5.0))],
                                      host_sample=256, seed=11 + precision)
    assert compared == 512 and installed >= 256          # (flights longer than Tmax are compared, not installed)


@gpu
def test_gpu_parity_all_combos():
    case_parity(None, 64, Tmax=2400, host_sample=16)


@gpu
def test_gpu_slot_isolation():
    case_slot_isolation(None, 1024)


@gpu
def test_gpu_mask_none_picks_finished():
    case_mask_none_picks_finished(None, 1024)


@gpu
def test_gpu_errors():
    case_errors(None, 1024)


@gpu
def test_gpu_closed_loop_vs_oracle():
    worst, flights, after = case_closed_loop_vs_oracle(None, 64, 200)
    print(f"closed loop: worst deviation {worst:.2e}, {flights} flights replanned")
    assert flights >= 64


@gpu
def test_gpu_checkpoint_after_replans():
    case_checkpoint(None, 256)

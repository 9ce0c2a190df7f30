"""The device trainer (mpcq_rgp_train / mpcq_record_train): drag models trained on all samples of a stream in one launch, from caller
arrays or from a recording's drag field in place.  The same cases run on the lane emulator (CPU) and on the MI355X (-m gpu, the
product library).  Yardsticks: vectors made by importing the reference's RGP.py (tests/golden/rgp_vectors.npz, learn_vectors.npz), the
stepwise learner (Learner.step, OracleLearner), the engine's own recorded flight, and the numpy restatement of RGP.regress below.

Tolerances (the project's own): REGRESS 1e-10 max(1, max|ref|) (DESIGN.md section 1 row a7 holds the RGP state to this figure against the
imported RGP.py); LEARN 1e-8 max(1, max|ref|) and 1e-7 max|K_x^-1| for the inverse (the bounds of rgp_learn_matches_reference_streams).
Every case prints the worst deviation seen in front of its assertion (DESIGN.md section 16 quotes them)."""
import ctypes
import gc
import os
import subprocess

import numpy as np
import pytest

from helpers import load_golden
from mpc_quad_ros_amd import _lib
from mpc_quad_ros_amd.engine import Engine, Learner
from mpc_quad_ros_amd.params import rgp_basis_linspace
from test_record import config, expect_rc, new_engine, same, snapshot

EMU_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "wave_emu")
EMU = os.path.join(EMU_DIR, "libmpcq_emu.so")
MPCQ_ERR_INVALID, MPCQ_ERR_DEVICE, MPCQ_ERR_STATE = -1, -2, -3
TOL_R, TOL_L, TOL_KI = 1e-10, 1e-8, 1e-7
REC = ("drag", "rgp_mu", "rgp_C")
WORST = {}


@pytest.fixture(scope="module")
def emu():
    subprocess.check_call(["make", "-C", EMU_DIR], stdout=subprocess.DEVNULL)
    return EMU


def close_to(tag, got, ref, tol, scale=None):
    """|got - ref| <= tol * scale (default max(1, max|ref|)), the figure printed in front of the assertion."""
    scale = max(1.0, np.abs(ref).max()) if scale is None else scale
    dev = np.abs(got - ref).max() / scale
    key = "regress" if tol == TOL_R else ("Kx_inv" if tol == TOL_KI else "learn")
    WORST[key] = max(WORST.get(key, 0.0), dev)
    print(f"{tag}: deviation {dev:.3e} (scaled; bound {tol:g}); worst so far {WORST}")
    assert got.shape == ref.shape and dev <= tol, (tag, dev)


def streams(s, S=2):
    """a scalar stream [T] as [S, T, 3]: every regressor sees the same samples"""
    return np.tile(np.asarray(s)[None, :, None], (S, 1, 3))


# ------------------------------------------------------------------ the yardstick: numpy restatement of RGP.regress over a stream
def np_regress(basis, theta, v, a):
    """basis [3,nb], theta [3,3], v, a [S,T,3] -> mu [S,3,nb], C [S,3,nb,nb] (src/gp/RGP.py:303-330, from mu = 0, C = K_x)."""
    S, T, nb = v.shape[0], v.shape[1], basis.shape[1]
    mu, C = np.zeros((S, 3, nb)), np.zeros((S, 3, nb, nb))
    for d in range(3):
        L, sf, sn = theta[d]
        X = basis[d]
        Kx = sf ** 2 * np.exp(-0.5 * (X[:, None] - X[None, :]) ** 2 / L ** 2) + sn ** 2 * np.eye(nb)
        Ki = np.linalg.inv(Kx)
        for s in range(S):
            m, Cs = np.zeros(nb), Kx.copy()
            for t in range(T):
                ks = sf ** 2 * np.exp(-0.5 * (v[s, t, d] - X) ** 2 / L ** 2)
                J = ks @ Ki
                G = Cs @ J / (sf ** 2 - J @ ks + J @ Cs @ J + sn ** 2)
                m = m + G * (a[s, t, d] - J @ m)
                Cs = Cs - np.outer(G, J @ Cs)
            mu[s, d], C[s, d] = m, Cs
    return mu, C


def lds_bytes(nb, learn, rc, rk):
    """the trainer's LDS per workgroup (mpcq_train.hpp: layout)"""
    npp = nb + 4
    scr = npp * npp + max(7 * npp, 2 * nb * nb) + 5 * nb + 2 * (nb + 2) + 34 if learn else 4 * nb
    return 8 * ((rc + rk) * nb * nb + nb + 12 + nb + scr)


class lds_limit:
    """MPCQ_TRAIN_LDS_BYTES for the calls inside: the residency arms at any basis size"""
    def __init__(self, n): self.n = n
    def __enter__(self): os.environ["MPCQ_TRAIN_LDS_BYTES"] = str(self.n)
    def __exit__(self, *a): del os.environ["MPCQ_TRAIN_LDS_BYTES"]


# ------------------------------------------------------------------ cases (engine library)
def case_reference_regress(lib):
    """1. RGP.regress streams of the imported RGP.py: the last state, and the first (T = 1: an off-by-one in the sample walk)."""
    v = load_golden("rgp_vectors.npz")
    e = Engine(config(2), lib_path=lib)
    for c in range(int(v["ncases"])):
        p = f"c{c}_"
        X, theta, s, y = v[p + "X"], v[p + "theta"], v[p + "s"], v[p + "y"]
        r = e.rgp_train(streams(s), streams(y), basis=np.tile(X, (3, 1)), theta=np.tile(theta, (3, 1)))
        assert sorted(r) == ["C_g", "mu_g"]
        ref_mu, ref_C = (np.broadcast_to(x, (2, 3) + x.shape) for x in (v[p + "mu"][-1], v[p + "C_last"]))
        close_to(f"regress case {c} nb={len(X)} mu", r["mu_g"], ref_mu, TOL_R)
        close_to(f"regress case {c} C", r["C_g"], ref_C, TOL_R)
        r = e.rgp_train(streams(s[:1]), streams(y[:1]), basis=np.tile(X, (3, 1)), theta=theta)
        close_to(f"regress case {c} T=1 mu", r["mu_g"], np.broadcast_to(v[p + "mu"][0], r["mu_g"].shape), TOL_R)
        close_to(f"regress case {c} T=1 C", r["C_g"], np.broadcast_to(v[p + "C_first"], r["C_g"].shape), TOL_R)
    e.close()


def case_reference_learn(lib):
    """2. RGP.learn streams of the imported RGP.py: the last joint state, K_x^-1, and the prefixes whose covariance the vectors hold."""
    v = load_golden("learn_vectors.npz")
    e = Engine(config(2), lib_path=lib)
    for c in range(int(v["ncases"])):
        p = f"c{c}_"
        nb, X, theta, s, y = int(v[p + "nb"]), v[p + "X"], v[p + "theta"], v[p + "s"], v[p + "y"]
        steps = [int(k) for k in v[p + "C_z_steps"]]
        assert steps[-1] == len(s) - 1
        for i, k in enumerate(steps):          # step k = the first k + 1 samples
            r = e.rgp_train(streams(s[:k + 1]), streams(y[:k + 1]), mode="learn", basis=np.tile(X, (3, 1)), theta=theta)
            mu_z, Cz = v[p + "mu_z"][k], v[p + "C_z"][i]
            bc = lambda x, like: np.broadcast_to(x, like.shape)
            close_to(f"learn case {c} nb={nb} step {k} mu_g", r["mu_g"], bc(mu_z[:nb], r["mu_g"]), TOL_L, max(1.0, np.abs(mu_z).max()))
            close_to(f"learn case {c} step {k} mu_eta", r["mu_eta"], bc(mu_z[nb:], r["mu_eta"]), TOL_L, max(1.0, np.abs(mu_z).max()))
            close_to(f"learn case {c} step {k} C_g", r["C_g"], bc(Cz[:nb, :nb], r["C_g"]), TOL_L, max(1.0, np.abs(Cz).max()))
            close_to(f"learn case {c} step {k} C_eta", r["C_eta"], bc(Cz[nb:, nb:], r["C_eta"]), TOL_L, max(1.0, np.abs(Cz).max()))
        Ki = v[p + "K_x_inv_last"]
        close_to(f"learn case {c} K_x^-1", r["K_x_inv"], np.broadcast_to(Ki, r["K_x_inv"].shape), TOL_KI, np.abs(Ki).max())
    e.close()


def case_equals_stepwise(lib):
    """3. One launch over 12 samples against Learner.step x 12 (B = 5, nb = 12, different streams and thetas), in every residency arm;
    then nb = 64, where C_g is resident and K_x^-1 is not, against OracleLearner."""
    from oracle.oracle import OracleLearner
    rng = np.random.default_rng(3)
    B, nb, T = 5, 12, 12
    basis = np.tile(np.linspace(-12, 12, nb), (3, 1))
    theta = np.array([[1.0, 0.1, 0.1], [2.0, 0.5, 0.05], [1.5, 0.3, 0.2]])
    e = Engine(config(2), lib_path=lib)
    a = Learner(B, basis, theta, lib_path=lib)
    sv, yv = np.zeros((B, T, 3)), np.zeros((B, T, 3))
    for k in range(T):
        sv[:, k] = rng.uniform(-10, 10, (B, 3)); yv[:, k] = 0.3 * sv[:, k] + rng.normal(0, 0.1, (B, 3))
        a.step(sv[:, k], yv[:, k])
    ga = a.get()
    a.close()
    r = e.rgp_train(sv, yv, mode="learn", basis=basis, theta=theta)
    assert sorted(r) == sorted(ga)
    for key in ga:
        close_to(f"one launch against Learner.step x {T}: {key}", r[key], ga[key], TOL_KI if key == "K_x_inv" else TOL_L,
                 np.abs(ga[key]).max() if key == "K_x_inv" else None)
    print("bit-identical to the stepwise learner:", {key: bool(np.array_equal(r[key], ga[key])) for key in ga})
    # the residency arms compute the same numbers: C_g alone resident, neither resident; less LDS than the smallest layout: refused
    both, conly, neither = (lds_bytes(nb, True, *arm) for arm in ((1, 1), (1, 0), (0, 0)))
    assert both > conly > neither
    for limit in (conly, neither):
        with lds_limit(limit):
            r2 = e.rgp_train(sv, yv, mode="learn", basis=basis, theta=theta)
        for key in r:
            assert np.array_equal(r[key], r2[key]), (limit, key)
    with lds_limit(neither - 8):
        expect_rc(MPCQ_ERR_DEVICE, e.rgp_train, sv, yv, mode="learn", basis=basis, theta=theta)
    rr = e.rgp_train(sv, yv, basis=basis, theta=theta)
    with lds_limit(lds_bytes(nb, False, 1, 0)):
        r1 = e.rgp_train(sv, yv, basis=basis, theta=theta)
    with lds_limit(lds_bytes(nb, False, 0, 0)):
        r0 = e.rgp_train(sv, yv, basis=basis, theta=theta)
    for key in rr:
        assert np.array_equal(rr[key], r1[key]) and np.array_equal(rr[key], r0[key]), key
    # nb = 64: the scratch and C_g fit a workgroup's 160 KB, K_x^-1 on top of them does not
    assert lds_bytes(64, True, 1, 1) > 160 * 1024 >= lds_bytes(64, True, 1, 0)
    B, nb, T = 2, 64, 6
    basis = np.tile(np.linspace(-12, 12, nb), (3, 1))
    o = OracleLearner(B, basis, theta)
    sv, yv = np.zeros((B, T, 3)), np.zeros((B, T, 3))
    for k in range(T):
        sv[:, k] = rng.uniform(-10, 10, (B, 3)); yv[:, k] = 0.3 * sv[:, k] + rng.normal(0, 0.1, (B, 3))
        o.step(sv[:, k], yv[:, k])
    go = o.get()
    r = e.rgp_train(sv, yv, mode="learn", basis=basis, theta=theta)
    for key in go:
        close_to(f"nb = 64 against OracleLearner: {key}", r[key], go[key], TOL_KI if key == "K_x_inv" else TOL_L,
                 np.abs(go[key]).max() if key == "K_x_inv" else None)
    e.close()


def fly(lib, B, K, quads=None, fields=REC, capacity=None, **kw):
    e = new_engine(lib, B, **kw)
    e.record_start(quads=quads, fields=fields, every=1, capacity=capacity or K)
    e.sim_steps(K, 2, 5e-3)
    assert e.record_info()[0] == K
    return e


def case_flight_retrains_to_itself(lib):
    """4. REGRESS on the engine's own model over the recorded rows 0..k reproduces the recorded RGP state of row k."""
    B, K = 3, 30
    e = fly(lib, B, K)
    rec = e.record_get()
    assert np.abs(rec["a_drag"]).max() > 0 and np.abs(rec["rgp_mu_g_t"][:, -1]).max() > 0
    for k in (K - 1, 0, 7):
        r = e.record_train(rows=(0, k + 1))
        close_to(f"rows 0..{k} mu", r["mu_g"], rec["rgp_mu_g_t"][:, k], TOL_R)
        close_to(f"rows 0..{k} C", r["C_g"], rec["rgp_C_g_t"][:, k], TOL_R)
    full = e.record_train()
    assert np.array_equal(full["mu_g"], e.record_train(rows=(0, K))["mu_g"])
    again = e.rgp_train(rec["v_body"], rec["a_drag"])            # one routine serves both entry points
    assert np.array_equal(again["mu_g"], full["mu_g"]) and np.array_equal(again["C_g"], full["C_g"])
    # the result loads into a fresh engine of the model with set_state
    xq = np.tile(np.linspace(-20, 19.5, 80), (3, 1))
    fresh = Engine(config(B), lib_path=lib)
    fresh.set_state(mu=full["mu_g"], C=full["C_g"])
    (m1, v1), (m0, v0) = fresh.rgp_predict(xq), e.rgp_predict(xq)
    close_to("predict from the retrained state: mean", m1, m0, TOL_R)
    close_to("predict from the retrained state: var", v1, v0, TOL_R, 0.1 ** 2)
    fresh.close(); e.close()


def case_another_model(lib):
    """5. nb = 20, theta = [3, .1, .01] from the flight of an nb = 10 engine; pair_next; a row window; a subset in caller order."""
    B, K, quads = 3, 30, np.array([2, 0])
    e = fly(lib, B, K, quads=quads, fields=("drag",))
    rec = e.record_get()
    v, a = rec["v_body"], rec["a_drag"]
    assert v.shape == (2, K, 3) and not np.array_equal(v[0], v[1])
    basis, theta = rgp_basis_linspace(12.0, 20), np.tile([3.0, 0.1, 0.01], (3, 1))
    kw = dict(basis=basis, theta=[3.0, 0.1, 0.01])
    plain = e.record_train(**kw)
    for key, ref in zip(("mu_g", "C_g"), np_regress(basis, theta, v, a)):       # streams in the caller's order [2, 0]
        close_to(f"another model {key}", plain[key], ref, TOL_R)
    nxt = e.record_train(pair_next=True, **kw)
    assert not np.array_equal(nxt["mu_g"], plain["mu_g"])
    for key, ref in zip(("mu_g", "C_g"), np_regress(basis, theta, v[:, :-1], a[:, 1:])):
        close_to(f"another model, pair_next {key}", nxt[key], ref, TOL_R)
    win = e.record_train(rows=(5, 10), **kw)
    for key, ref in zip(("mu_g", "C_g"), np_regress(basis, theta, v[:, 5:15], a[:, 5:15])):
        close_to(f"another model, rows 5..14 {key}", win[key], ref, TOL_R)
    winn = e.record_train(rows=(5, 10), pair_next=True, **kw)
    for key, ref in zip(("mu_g", "C_g"), np_regress(basis, theta, v[:, 5:14], a[:, 6:15])):
        close_to(f"another model, rows 5..14 pair_next {key}", winn[key], ref, TOL_R)
    both = e.rgp_train(v, a, pair_next=True, **kw)
    assert np.array_equal(both["mu_g"], nxt["mu_g"]) and np.array_equal(both["C_g"], nxt["C_g"])
    lr = e.record_train(mode="learn", **kw)                     # LEARN from the recording = LEARN from its samples
    lc = e.rgp_train(v, a, mode="learn", **kw)
    for key in lr:
        assert np.array_equal(lr[key], lc[key], equal_nan=True), key
    e.close()


def raw(e, mode=1, pair_next=0, nb=0, basis=None, theta=None, outs=("mu",), S=None, T=None, v=None, a=None, rows=None, spec=True, out=True):
    """a call through the C ABI with arguments the Python layer would refuse: the return code"""
    n = nb if nb > 0 else max(e.nb, 1)
    Sx = 8
    arrays = dict(mu=np.zeros((Sx, 3, n)), C=np.zeros((Sx, 3, n, n)), mu_eta=np.zeros((Sx, 3, 3)), C_eta=np.zeros((Sx, 3, 3, 3)), Kx_inv=np.zeros((Sx, 3, n, n)))
    sp = _lib.TrainSpec(mode=mode, pair_next=pair_next, nb=nb, basis=_lib.d(basis), theta=_lib.d(theta))
    o = _lib.TrainOut(**{k: _lib.d(arrays[k]) for k in outs})
    sp_, o_ = (ctypes.byref(sp) if spec else None), (ctypes.byref(o) if out else None)
    if rows is not None:
        return e.lib.mpcq_record_train(e.h, sp_, rows[0], rows[1], o_)
    return e.lib.mpcq_rgp_train(e.h, sp_, _lib.d(v), _lib.d(a), S, T, o_)


def case_state_and_arguments(lib):
    """6. Every error rule returns its code and leaves engine and recording as they were; NaN samples; mission and scoreboard
    read-outs; an MPCQ_PRECISION_F32 engine."""
    B, K = 3, 6
    e = fly(lib, B, K, capacity=16)
    wp = e.sim_get_state()[0][:, None, None, 0:3] + np.array([[0.5, 0, 0], [1.0, 0.5, 0]])[None, None]
    e.mission_set(wp, 12.0, 12.0)
    e.score_start(2)
    e.sim_steps(2, 2, 5e-3)
    K += 2
    before, rec0, ms0, sc0 = snapshot(e), e.record_get(), e.mission_get(), e.score_get()
    v, a = np.ones((2, 4, 3)), np.ones((2, 4, 3))
    X20, th = rgp_basis_linspace(12.0, 20), np.tile([3.0, 0.1, 0.01], (3, 1))
    ok = dict(S=2, T=4, v=v, a=a)
    bad_L = th.copy(); bad_L[1, 0] = 0.0
    I, St = MPCQ_ERR_INVALID, MPCQ_ERR_STATE
    for want, kw in ((I, dict(spec=False)), (I, dict(out=False)), (I, dict(outs=())), (I, dict(mode=0)), (I, dict(mode=3)), (I, dict(nb=-1)),
                     (I, dict(nb=65, basis=np.zeros((3, 65)), theta=th)), (I, dict(nb=20, basis=X20)), (I, dict(nb=20, theta=th)),
                     (I, dict(basis=X20)), (I, dict(theta=th)), (I, dict(nb=20, basis=X20, theta=bad_L)),
                     (I, dict(mode=2, nb=20, basis=X20, theta=bad_L)), (I, dict(outs=("mu", "mu_eta"))), (I, dict(outs=("C_eta",))),
                     (I, dict(outs=("mu", "Kx_inv"))), (I, dict(pair_next=2))):
        assert raw(e, **{**ok, **kw}) == want, kw
        assert raw(e, rows=(0, 2), **kw) == want, kw
    for kw in (dict(S=0), dict(S=-1), dict(T=0), dict(T=1, pair_next=1), dict(v=None), dict(a=None)):
        assert raw(e, **{**ok, **kw}) == I, kw
    for rows in ((-1, 1), (0, 0), (0, K + 1), (K, 1), (K - 1, 2), (0, -1)):
        assert raw(e, rows=rows) == I, rows
    assert raw(e, rows=(0, 1), pair_next=1) == I and raw(e, rows=(0, 2), pair_next=1) == 0
    assert raw(e, **ok) == 0 and raw(e, mode=2, outs=("mu", "C", "mu_eta", "C_eta", "Kx_inv"), **ok) == 0
    assert raw(e, rows=(0, K)) == 0 and raw(e, rows=(K - 1, 1), mode=2, outs=("Kx_inv",)) == 0
    expect_rc(MPCQ_ERR_INVALID, e.record_train, rows=(0, K + 1))
    # a NaN sample in one stream poisons that stream's three regressors and no other
    rec = e.record_get()
    vn, an = rec["v_body"].copy(), rec["a_drag"].copy()
    clean = {m: e.rgp_train(vn, an, mode=m) for m in ("regress", "learn")}
    vn[1, 3, :] = np.nan
    for m in ("regress", "learn"):
        r = e.rgp_train(vn, an, mode=m)
        for key in r:
            assert np.isnan(r[key][1]).all(), (m, key)
            assert np.array_equal(r[key][[0, 2]], clean[m][key][[0, 2]]) and np.isfinite(r[key][[0, 2]]).all(), (m, key)
    vn[1, 3, :] = rec["v_body"][1, 3, :]
    an[2, 0, 1] = np.inf                                         # one axis: that regressor alone
    r = e.rgp_train(vn, an)
    assert not np.isfinite(r["mu_g"][2, 1]).any() and np.array_equal(r["mu_g"][2, [0, 2]], clean["regress"]["mu_g"][2, [0, 2]])
    # nothing above changed the engine, the recording, the mission or the scoreboard
    same(before, snapshot(e), before.keys())
    same(rec0, e.record_get())
    ms1, sc1 = e.mission_get(), e.score_get()
    for k0, k1 in ((ms0, ms1), (sc0, sc1)):
        for key in k0:
            assert np.array_equal(np.asarray(k0[key]), np.asarray(k1[key]), equal_nan=True), key
    twin = fly(lib, B, K - 2, capacity=16)                                    # and the flight goes on as the twin's that never trained
    twin.mission_set(wp, 12.0, 12.0); twin.score_start(2)
    twin.sim_steps(2, 2, 5e-3)
    for x in (e, twin):
        x.sim_steps(3, 2, 5e-3)
    same(snapshot(e), snapshot(twin), before.keys())
    twin.close()
    e.record_stop()
    assert raw(e, rows=(0, 1)) == St                             # no active recording
    expect_rc(MPCQ_ERR_STATE, e.record_train)
    e.record_start(fields=("x_odom", "rgp_mu"), capacity=4)
    e.sim_steps(2, 2, 5e-3)
    assert raw(e, rows=(0, 1)) == I                              # drag not recorded
    e.close()
    n0 = Engine(config(B, nb=0), lib_path=lib)
    assert raw(n0, **ok) == St and raw(n0, nb=20, basis=X20, theta=th, **ok) == 0
    n0.close()
    fixed = Engine(config(B, static_gp=True), lib_path=lib)     # a static-GP engine has a basis: its own model trains
    assert raw(fixed, **ok) == 0 and raw(fixed, mode=2, **ok) == 0
    fixed.close()
    # an MPCQ_PRECISION_F32 engine trains in double on its double drag field
    f = fly(lib, 2, 5, fields=("drag",), precision=1)
    rec = f.record_get()
    for m in ("regress", "learn"):
        r, r2 = f.record_train(mode=m), f.rgp_train(rec["v_body"], rec["a_drag"], mode=m)
        for key in r:
            assert r[key].dtype == np.float64 and np.isfinite(r[key]).all() and np.array_equal(r[key], r2[key]), (m, key)
    assert np.abs(r["mu_g"]).max() > 0
    f.close()


def case_close_releases_everything(lib):
    """7. close() after both entry points, both modes and a caller's model: the emulator's count of live allocations is back."""
    live = _lib.load(lib).mpcq_emu_live
    live.restype = ctypes.c_long
    gc.collect()
    before = live()
    e = fly(lib, 3, 4)
    rec = e.record_get()
    e.record_train(); e.record_train(mode="learn", rows=(1, 2))
    e.rgp_train(rec["v_body"], rec["a_drag"], mode="learn", basis=rgp_basis_linspace(12.0, 20), theta=[3.0, 0.1, 0.01])
    e.rgp_train(np.tile(rec["v_body"], (4, 3, 1)), np.tile(rec["a_drag"], (4, 3, 1)))      # the scratch grows
    assert live() > before
    e.close()
    assert live() == before, live() - before


CASES = [case_reference_regress, case_reference_learn, case_equals_stepwise, case_flight_retrains_to_itself, case_another_model,
         case_state_and_arguments]
IDS = [c.__name__[5:] for c in CASES]


# ------------------------------------------------------------------ lane emulator (CPU)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_emu(emu, case):
    case(emu)


def test_emu_close_releases_everything(emu):
    case_close_releases_everything(emu)


# ------------------------------------------------------------------ MI355X
@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_gpu(case):
    case(None)


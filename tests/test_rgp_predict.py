"""The RGP read-out (mpcq_rgp_predict / mpcq_record_predict): posterior mean and variance of every quadrotor's learned drag model at
query points, evaluated on the device.  The same cases run on the lane emulator (CPU, small batches) and on the MI355X (-m gpu, the
product library).  Yardsticks: vectors of the reference's RGP.predict / GP.predict (tests/golden/rgp_predict_vectors.npz, made by
tests/golden/make_predict_golden.py) and the numpy restatement below applied to what get_rgp() returns.

Tolerance (DESIGN.md section 1 row a7 holds the RGP state to 1e-10 against the imported RGP.py; the same figure here):
|mean - ref| <= 1e-10 max(1, max|ref mean|) and |var - ref| <= 1e-10 sigma_f^2 per case.  A plain-loop fp64 restatement with another
summation order deviates from RGP.predict by <= 1.4e-14 / 4e-15 sigma_f^2 on these states, so four orders of magnitude remain for the
engine's own K_x^-1 and the device's order."""
import os
import subprocess

import numpy as np
import pytest

from helpers import load_golden
from mpc_quad_ros_amd import _lib
from mpc_quad_ros_amd.engine import Engine
from mpc_quad_ros_amd.params import EngineConfig, hummingbird, static_gp_theta
from test_record import config, expect_rc, new_engine, same, snapshot

EMU_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "wave_emu")
EMU = os.path.join(EMU_DIR, "libmpcq_emu.so")
MPCQ_ERR_INVALID, MPCQ_ERR_STATE = -1, -3
TOL = 1e-10
GRID = np.arange(-20, 20, 0.5)
WORST = {}      # largest deviations seen, printed by the cases (DESIGN.md section 12 quotes them)


@pytest.fixture(scope="module")
def emu():
    subprocess.check_call(["make", "-C", EMU_DIR], stdout=subprocess.DEVNULL)
    return EMU


# ------------------------------------------------------------------ the yardstick: numpy restatement of RGP.predict / GP.predict
def np_predict(basis, theta, mu, C, xq):
    """basis [3,nb], theta [3,3] = (L, sigma_f, sigma_n) per axis, mu [B,3,nb], C [B,3,nb,nb] or None (static GP: no J C J^T term),
    xq [3,M] or [B,3,M] -> mean, var [B,3,M] (src/gp/RGP.py:199-210)."""
    B = mu.shape[0]
    xq = np.broadcast_to(xq, (B,) + xq.shape[-2:])
    mean, var = np.zeros(xq.shape), np.zeros(xq.shape)
    for d in range(3):
        L, sf, sn = theta[d]
        X = basis[d]
        Kx = sf ** 2 * np.exp(-0.5 * (X[:, None] - X[None, :]) ** 2 / L ** 2) + sn ** 2 * np.eye(len(X))
        ks = sf ** 2 * np.exp(-0.5 * (xq[:, d, :, None] - X[None, None, :]) ** 2 / L ** 2)          # [B,M,nb]
        J = ks @ np.linalg.inv(Kx)
        mean[:, d] = np.einsum("bmi,bi->bm", J, mu[:, d])
        var[:, d] = sf ** 2 - np.einsum("bmi,bmi->bm", J, ks)
        if C is not None:
            var[:, d] += np.einsum("bmi,bij,bmj->bm", J, C[:, d], J)
    return mean, var


def theta3(theta):
    th = np.asarray(theta, dtype=np.float64)
    return np.tile(th, (3, 1)) if th.ndim == 1 else th


def check(tag, mean, var, rmean, rvar, sf2):
    """Per axis: the issue's bounds, with the figures printed in front of the assertion."""
    for d in range(3):
        em = np.abs(mean[:, d] - rmean[:, d]).max() / max(1.0, np.abs(rmean[:, d]).max())
        ev = np.abs(var[:, d] - rvar[:, d]).max() / sf2[d]
        WORST["mean"] = max(WORST.get("mean", 0.0), em); WORST["var"] = max(WORST.get("var", 0.0), ev)
        print(f"{tag} axis {d}: mean deviation {em:.3e} (scaled), var deviation {ev:.3e} sigma_f^2; worst so far {WORST}")
        assert em <= TOL and ev <= TOL, (tag, d, em, ev)


# ------------------------------------------------------------------ cases (engine library, ...)
def case_reference_vectors(lib, B=6):
    """1. States of the reference's RGP loaded with set_state; three fixture cases of equal nb on the three axes, K by quadrotor."""
    g = load_golden("rgp_predict_vectors.npz")
    Ks = [int(k) for k in g["Ks"]]
    for cases in ((0, 1, 5), (2, 4, 2), (3, 3, 3)):
        nb = len(g[f"r{cases[0]}_0_X"])
        basis = np.stack([g[f"r{c}_0_X"] for c in cases])
        theta = np.stack([g[f"r{c}_0_theta"] for c in cases])
        e = Engine(EngineConfig(batch=B, N=10, T=1.0, quad=hummingbird(), nb=nb, dt_pred=0.01, basis=basis, theta=theta), lib_path=lib)
        key = lambda b, d, name: g[f"r{cases[d]}_{Ks[b % 3]}_{name}"]
        stack = lambda name: np.stack([np.stack([key(b, d, name) for d in range(3)]) for b in range(B)])
        mu, C, xq, rmean, rvar, rstd = (stack(n) for n in ("mu", "C", "xq", "mean", "var", "std"))
        e.set_state(mu=mu, C=C)
        sf2 = theta[:, 1] ** 2
        mean, var = e.rgp_predict(xq, per_quad=True)                  # every (case, K) at its own 96 points
        check(f"vectors nb={nb} per-quadrotor points", mean, var, rmean, rvar, sf2)
        assert rvar.min() > 0 and np.isfinite(np.sqrt(var)).all()
        for d in range(3):      # d std = d var / (2 std): the variance bound carried through the square root
            assert np.abs(np.sqrt(var[:, d]) - rstd[:, d]).max() <= TOL * sf2[d] / (2 * rstd[:, d].min())
        mean, var = e.rgp_predict(np.tile(GRID, (3, 1)))              # the shared grid: the first 80 points of every vector
        check(f"vectors nb={nb} shared grid", mean, var, rmean[:, :, :80], rvar[:, :, :80], sf2)
        assert np.array_equal(e.rgp_predict(np.tile(GRID, (3, 1)), var=False), mean)
        e.close()
    for c in range(int(g["n_static"])):          # static GP (MPCQ_FLAG_STATIC_GP) against GP.predict
        v = load_golden("gp_vectors.npz")
        X, y, theta = v[f"c{c}_X"], v[f"c{c}_y"], v[f"c{c}_theta"]
        e = Engine(EngineConfig(batch=2, N=10, quad=hummingbird(), nb=len(X), basis=np.tile(X, (3, 1)), theta=static_gp_theta(theta), static_gp=True),
                   lib_path=lib)
        e.set_params(np.tile(np.tile(y, 3), (2, 1)))
        xq = np.tile(g[f"s{c}_xq"], (3, 1))
        mean, var = e.rgp_predict(xq)
        rm, rv = (np.broadcast_to(g[f"s{c}_{n}"], (2, 3, xq.shape[1])) for n in ("mean", "var"))
        check(f"static case {c}", mean, var, rm, rv, np.full(3, theta[-2] ** 2))
        # C of a static engine is not read: poisoning it changes nothing
        e.set_state(C=np.full((2, 3, len(X), len(X)), np.nan))
        m2, v2 = e.rgp_predict(xq)
        assert np.array_equal(m2, mean) and np.array_equal(v2, var)
        e.close()


def case_fresh(lib, B, nb=10):
    """2. C_0 = K_x: mean exactly 0, var = sigma_f^2 within the bound (the two J terms cancel)."""
    e = Engine(config(B, nb=nb), lib_path=lib)
    mean, var = e.rgp_predict(np.tile(GRID, (3, 1)))
    sf2 = 0.1 ** 2
    print(f"fresh engine: |var - sigma_f^2| max {np.abs(var - sf2).max() / sf2:.3e} sigma_f^2")
    assert np.array_equal(mean, np.zeros((B, 3, 80))) and np.abs(var - sf2).max() <= TOL * sf2
    e.close()


def case_after_flying(lib, B, K, M=80, **kw):
    """3. After sim_steps: rgp_predict against the restatement applied to get_rgp() (a float engine against ITS get_rgp())."""
    e = new_engine(lib, B, **kw)
    e.sim_steps(K, 2, 5e-3)
    mu, C = e.get_rgp()
    assert np.abs(mu).max() > 0
    xq = np.tile(np.linspace(-20, 19.5, M), (3, 1))
    mean, var = e.rgp_predict(xq)
    th = theta3(e.cfg.theta)
    rm, rv = np_predict(np.asarray(e.cfg.basis), th, mu, C, xq)
    check(f"after {K} periods B={B} {kw}", mean, var, rm, rv, th[:, 1] ** 2)
    e.close()
    return mean, var


def case_shapes(lib, B, nb=10):
    """4. M = 1, 64, 65, 200, 4096; per_quad with the shared grid in every row equals the shared-grid call bit for bit."""
    e = new_engine(lib, B, nb=nb)
    e.sim_steps(3, 2, 5e-3)
    mu, C = e.get_rgp()
    th, basis = theta3(e.cfg.theta), np.asarray(e.cfg.basis)
    rng = np.random.default_rng(4)
    for M in (1, 64, 65, 200, 4096):
        xq = rng.uniform(-18, 18, (3, M))
        mean, var = e.rgp_predict(xq)
        assert mean.shape == var.shape == (B, 3, M)
        rm, rv = np_predict(basis, th, mu, C, xq)
        check(f"M={M}", mean, var, rm, rv, th[:, 1] ** 2)
        m2, v2 = e.rgp_predict(np.tile(xq, (B, 1, 1)), per_quad=True)
        assert np.array_equal(m2, mean) and np.array_equal(v2, var), M
    xq = rng.uniform(-18, 18, (B, 3, 70))
    mean, var = e.rgp_predict(xq, per_quad=True)
    rm, rv = np_predict(basis, th, mu, C, xq)
    check("per-quadrotor random points", mean, var, rm, rv, th[:, 1] ** 2)
    e.close()


def case_recording(lib, B, K, quads=None, every=1, window=None, M=80, **kw):
    """5. record_predict over a recording equals, bit for bit, rgp_predict after each period on a twin advanced with sim_steps(1)."""
    xq = np.tile(np.linspace(-20, 19.5, M), (3, 1))
    a = new_engine(lib, B, **kw)
    a.record_start(quads=quads, fields=("rgp_mu", "rgp_C"), every=every, capacity=K)
    a.sim_steps(K, 2, 5e-3)
    rows = a.record_info()[0]
    assert rows == (K + every - 1) // every
    mean, var = a.record_predict(xq, rows=window)
    assert np.array_equal(a.record_predict(xq, rows=window, var=False), mean)
    b = new_engine(lib, B, **kw)
    ms, vs = [], []
    for k in range(K):
        b.sim_steps(1, 2, 5e-3)
        if k % every == 0:
            m, v = b.rgp_predict(xq)
            ms.append(m); vs.append(v)
    sel = np.arange(B) if quads is None else np.asarray(quads)
    r0, nr = (0, rows) if window is None else window
    tm, tv = (np.swapaxes(np.stack(x), 0, 1)[sel][:, r0:r0 + nr] for x in (ms, vs))
    assert mean.shape == tm.shape == (len(sel), nr, 3, M)
    assert np.array_equal(mean, tm) and np.array_equal(var, tv)
    assert np.abs(mean).max() > 0
    # mean alone needs only the mean field
    a.record_stop()
    a.record_start(fields=("rgp_mu",), capacity=2)
    a.sim_steps(1, 2, 5e-3)
    assert a.record_predict(xq, var=False).shape == (B, 1, 3, M)
    expect_rc(MPCQ_ERR_INVALID, a.record_predict, xq)          # var without rgp_C
    a.close(); b.close()


def case_no_side_effects(lib, B):
    """6. Both calls leave the engine bit-identical, and the flight that follows equals the twin's that never asked."""
    xq = np.tile(GRID, (3, 1))
    a, b = new_engine(lib, B), new_engine(lib, B)
    for e in (a, b):
        e.record_start(fields=("rgp_mu", "rgp_C", "x_odom"), capacity=20)
        e.sim_steps(4, 2, 5e-3)
    before = snapshot(a)
    a.rgp_predict(xq); a.rgp_predict(np.tile(xq, (B, 1, 1)), per_quad=True); a.record_predict(xq, rows=(1, 2))
    same(before, snapshot(a), before.keys())
    for e in (a, b):
        e.sim_steps(4, 2, 5e-3)
    same(snapshot(a), snapshot(b), before.keys())
    same(a.record_get(), b.record_get())
    a.close(); b.close()


def case_errors(lib, B):
    """7. Every MPCQ_ERR_* rule of include/mpcq.h; a NaN query point gives NaN, status 0."""
    e = new_engine(lib, B)
    L = e.lib
    xq, out = np.zeros((3, 8)), np.zeros((B, 3, 8))
    P = L.mpcq_rgp_predict
    assert P(e.h, None, 8, 0, _lib.d(out), None) == MPCQ_ERR_INVALID
    assert P(e.h, _lib.d(xq), 8, 0, None, None) == MPCQ_ERR_INVALID
    for M in (0, -1, 4097):
        assert P(e.h, _lib.d(xq), M, 0, _lib.d(out), None) == MPCQ_ERR_INVALID
    for pq in (2, -1):
        assert P(e.h, _lib.d(xq), 8, pq, _lib.d(out), None) == MPCQ_ERR_INVALID
    assert P(e.h, _lib.d(xq), 8, 0, None, _lib.d(out)) == 0 and P(e.h, _lib.d(xq), 8, 0, _lib.d(out), None) == 0
    R = L.mpcq_record_predict
    assert R(e.h, _lib.d(xq), 8, 0, 1, _lib.d(out), None) == MPCQ_ERR_STATE            # no recording
    expect_rc(MPCQ_ERR_STATE, e.record_predict, xq)
    e.record_start(fields=("x_odom", "rgp_C"), capacity=10)
    e.sim_steps(3, 2, 5e-3)
    assert R(e.h, _lib.d(xq), 8, 0, 1, _lib.d(out), None) == MPCQ_ERR_INVALID          # rgp_mu not recorded
    e.record_stop()
    e.record_start(fields=("rgp_mu",), capacity=10)
    e.sim_steps(3, 2, 5e-3)
    assert R(e.h, _lib.d(xq), 8, 0, 1, _lib.d(out), None) == 0
    assert R(e.h, _lib.d(xq), 8, 0, 1, _lib.d(out), _lib.d(out)) == MPCQ_ERR_INVALID   # var without rgp_C
    e.record_stop()
    e.record_start(fields=("rgp_mu", "rgp_C"), capacity=10)
    assert R(e.h, _lib.d(xq), 8, 0, 1, _lib.d(out), None) == MPCQ_ERR_INVALID          # nothing recorded yet
    assert e.record_predict(xq)[0].shape == (B, 0, 3, 8)
    e.sim_steps(3, 2, 5e-3)
    for r0, nr in ((-1, 1), (0, 0), (0, 4), (3, 1), (2, 2), (0, -1)):
        assert R(e.h, _lib.d(xq), 8, r0, nr, _lib.d(out), None) == MPCQ_ERR_INVALID, (r0, nr)
    assert R(e.h, None, 8, 0, 1, _lib.d(out), None) == MPCQ_ERR_INVALID
    assert R(e.h, _lib.d(xq), 8, 0, 1, None, None) == MPCQ_ERR_INVALID
    assert R(e.h, _lib.d(xq), 4097, 0, 1, _lib.d(out), None) == MPCQ_ERR_INVALID
    assert R(e.h, _lib.d(xq), 8, 2, 1, _lib.d(out), _lib.d(np.zeros((B, 3, 8)))) == 0
    # NaN (and infinite) query points are no error
    xn = np.tile(np.array([0.5, np.nan, -3.0, np.inf]), (3, 1))
    mean, var = e.rgp_predict(xn)
    assert np.isnan(mean[:, :, 1]).all() and np.isnan(var[:, :, 1]).all()
    assert np.isfinite(mean[:, :, [0, 2, 3]]).all() and np.isfinite(var[:, :, [0, 2, 3]]).all()
    mean, var = e.record_predict(xn)
    assert np.isnan(mean[:, :, :, 1]).all() and np.isnan(var[:, :, :, 1]).all() and np.isfinite(mean[:, :, :, 0]).all()
    e.close()
    n0 = Engine(config(B, nb=0), lib_path=lib)
    assert P(n0.h, _lib.d(xq), 8, 0, _lib.d(out), None) == MPCQ_ERR_STATE
    n0.record_start()
    assert R(n0.h, _lib.d(xq), 8, 0, 1, _lib.d(out), None) == MPCQ_ERR_STATE
    n0.close()


def case_facade(lib, B):
    """8. quad_optimizer(...).gpe.predict mirrors GPEnsemble.predict; gpe.gp[d].predict one axis."""
    from mpc_quad_ros_amd.params import rgp_basis_linspace
    from mpc_quad_ros_amd.quad_opt import quad_optimizer
    q = quad_optimizer(t_horizon=1, n_nodes=10, gpe=dict(basis=rgp_basis_linspace(12.0, 10), theta=[1.0, 0.1, 0.1]), batch=B, lib_path=lib)
    rng = np.random.default_rng(8)
    q.regress_and_update_RGP_model([rng.uniform(-5, 5, B) for _ in range(3)], [rng.normal(0, 1, B) for _ in range(3)])
    X_t = [GRID, GRID + 0.1, GRID - 0.1]
    mu = q.gpe.predict(X_t)
    mu2, std = q.gpe.predict(X_t, std=True)
    assert isinstance(mu, list) and len(mu) == len(std) == 3 and all(m.shape == (B, 80) for m in mu + std)
    mean, var = q.engine.rgp_predict(np.stack(X_t))
    for d in range(3):
        assert np.array_equal(mu[d], mean[:, d]) and np.array_equal(mu2[d], mean[:, d])
        assert np.array_equal(std[d], np.sqrt(var[:, d])) and np.abs(std[d] ** 2 - var[:, d]).max() <= 4e-16 * np.abs(var[:, d]).max()
        m1, v1 = q.gpe.gp[d].predict(X_t[d], var=True)
        m1s, s1 = q.gpe.gp[d].predict(X_t[d], std=True)
        assert np.array_equal(m1, mean[:, d]) and np.array_equal(v1, var[:, d]) and np.array_equal(s1, std[d])
        assert np.array_equal(q.gpe.gp[d].predict(X_t[d]), mean[:, d]) and np.array_equal(m1s, m1)
    assert np.abs(mean).max() > 0
    with pytest.raises(AssertionError):
        q.gpe.predict(X_t[:2])
    with pytest.raises(AssertionError):
        q.gpe.predict([np.zeros((2, 2))] * 3)
    with pytest.raises(AssertionError):
        q.gpe.gp[0].predict(np.zeros((2, 2)))
    q.engine.close()


# ------------------------------------------------------------------ lane emulator (CPU)
def test_emu_reference_vectors(emu):
    case_reference_vectors(emu, B=3)


def test_emu_fresh_engine(emu):
    case_fresh(emu, 3)
    case_fresh(emu, 2, nb=20)


def test_emu_after_flying_both_precisions_and_groups(emu):
    a = case_after_flying(emu, 16, 6, tune=dict(groups=1))
    b = case_after_flying(emu, 16, 6, tune=dict(groups=2))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    case_after_flying(emu, 4, 6, precision=1)
    case_after_flying(emu, 2, 3, N=10, nb=50)


def test_emu_large_basis_reads_C_through_the_cache(emu):
    """nb > 64: C and K_x^-1 are not staged in LDS; the same arithmetic."""
    case_after_flying(emu, 2, 2, nb=70, M=70)


def test_emu_shapes_and_per_quadrotor_points(emu):
    case_shapes(emu, 3)


def test_emu_recording_bit_identical_to_live(emu):
    case_recording(emu, 6, 8)
    case_recording(emu, 6, 9, quads=np.array([4, 0, 5, 2]), window=(1, 2), every=3)
    case_recording(emu, 16, 6, quads=np.array([9, 2, 15, 7, 8]), window=(2, 3), tune=dict(groups=2))
    case_recording(emu, 3, 4, precision=1)


def test_emu_no_side_effects(emu):
    case_no_side_effects(emu, 5)


def test_emu_errors(emu):
    case_errors(emu, 3)


def test_emu_facade(emu):
    case_facade(emu, 3)


# ------------------------------------------------------------------ MI355X
gpu = pytest.mark.gpu


@gpu
def test_gpu_reference_vectors():
    case_reference_vectors(None, B=96)


@gpu
def test_gpu_fresh_engine():
    case_fresh(None, 1024)
    case_fresh(None, 64, nb=50)


@gpu
def test_gpu_after_flying_b1024_both_precisions_and_groups():
    a = case_after_flying(None, 1024, 20, tune=dict(groups=1))
    b = case_after_flying(None, 1024, 20, tune=dict(groups=2))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    case_after_flying(None, 1024, 20, precision=1)


@gpu
def test_gpu_after_flying_b8192():
    case_after_flying(None, 8192, 10, N=20, tune=dict(groups=2))
    case_after_flying(None, 8192, 10, N=20, precision=1)


@gpu
def test_gpu_after_flying_n50_nb50():
    case_after_flying(None, 512, 8, N=50, nb=50)
    case_after_flying(None, 512, 8, N=50, nb=50, precision=1)


@gpu
def test_gpu_large_basis_reads_C_through_the_cache():
    case_after_flying(None, 64, 3, nb=70, M=70)


@gpu
def test_gpu_shapes_and_per_quadrotor_points():
    case_shapes(None, 256)
    case_shapes(None, 32, nb=50)


@gpu
def test_gpu_recording_bit_identical_to_live():
    case_recording(None, 1024, 20)
    quads = np.array([1000, 3, 256, 255, 767, 768, 512, 511, 0, 1023])
    case_recording(None, 1024, 21, quads=quads, window=(2, 3), every=3, tune=dict(groups=4))
    case_recording(None, 512, 8, precision=1)
    case_recording(None, 128, 6, N=50, nb=50, window=(1, 4))


@gpu
def test_gpu_no_side_effects():
    case_no_side_effects(None, 1024)


@gpu
def test_gpu_errors():
    case_errors(None, 256)


@gpu
def test_gpu_facade():
    case_facade(None, 64)

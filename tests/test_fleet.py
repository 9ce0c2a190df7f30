"""The fleet (mpcq_fleet_set / _get / _stop, Engine.fleet_*, params.fleet_*): every quadrotor its own plant -- mass, inertia, thrust, geometry,
drag, payload, rotor functionality and a disturbance window -- while the controller keeps the engine's model.  The same cases run on the
lane emulator (CPU, small batches) and on the MI355X (-m gpu, the product library).  Shapes: N = 10, nb = 10, legacy_sim(), control period
0.1 s = 20 substeps of 5 ms, 8 periods or fewer.

Yardsticks:
 * the reference's own Quadrotor3D: tests/golden/plant_vectors.npz (make_plant_golden.py), 128 plants with every parameter drawn
   independently, 20 x one_step_forward with disturbances (cases 0..63) and 20 x update with inputs beyond [0, 1] (cases 64..127).
   Bound |x - x_ref| <= 1e-12 max(1, |x_ref|), the project's for this computation (test_engine_edges: the plant period against the
   reference's logs).  The device differs from the reference in operation order only (reciprocals of mass and J formed once, payload,
   f_d / mass and t_d / J added behind the shared derivative): a numpy restatement in that order stayed within 3.5e-15 scaled.
 * the fp64 oracle, one OracleEngine(batch = 1) per quadrotor with that quadrotor's constants, for the fields it knows (mass, J, thrust,
   geometry, drag): 1e-13 max(1, |x|), the project's bound for device plant against oracle plant.
 * the engine without a fleet, and the host loop that exists without the feature: bit for bit (np.array_equal; a fleet of default plants
   multiplies by 1.0 and adds 0.0, quadrotors are independent, and one kernel serves sim_steps and sim_plant_period)."""
import os
import re
import subprocess

import numpy as np
import pytest

from mpc_quad_ros_amd import _lib
from mpc_quad_ros_amd.engine import Engine
from mpc_quad_ros_amd.params import (PLANT_DTYPE, EngineConfig, QuadParams, fleet_defaults, fleet_drag_accel, fleet_sample, legacy_sim,
                                     rgp_basis_linspace)
from mpc_quad_ros_amd.trajectories import swarm_trajectories
from test_circle_mission import DT, assert_same, expect_rc, hover_slots, snapshot

HERE = os.path.dirname(os.path.abspath(__file__))
EMU_DIR = os.path.join(HERE, "wave_emu")
EMU = os.path.join(EMU_DIR, "libmpcq_emu.so")
GOLDEN = os.path.join(HERE, "golden", "plant_vectors.npz")
MPCQ_ERR_INVALID, MPCQ_ERR_STATE = -1, -3
NSUB, SIM_DT, CONTROL_DT = 20, 5e-3, 0.1
K = 8
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1
SAMPLE = dict(spread=1.3, payload_max=0.2, fault_prob=0.5, fault_min=0.6, gust_force=0.5, gust_torque=0.01, gust_window=(1, 4))


@pytest.fixture(scope="module")
def emu():
    subprocess.check_call(["make", "-C", EMU_DIR], stdout=subprocess.DEVNULL)
    return EMU


def config(B, **kw):
    return EngineConfig(batch=B, N=10, T=1.0, quad=legacy_sim(), nb=10, basis=rgp_basis_linspace(12.0, 10), theta=[1.0, 0.1, 0.1], dt_pred=0.01, **kw)


def golden_plants(n):
    """(plants [n] of the golden, x0, u, x_ref)."""
    g = np.load(GOLDEN, allow_pickle=False)
    p = np.zeros(n, PLANT_DTYPE)
    for name in PLANT_DTYPE.names:
        if name in g.files:
            p[name] = g[name][:n]
    p["d_from"], p["d_to"] = 0, 1          # one plant update, in fleet period 0
    assert float(g["g"]) == legacy_sim().g and int(g["n_sub"]) == NSUB and float(g["sim_dt"]) == SIM_DT
    return g, p


_SWARM = {}


def swarm(B):
    """Closed-loop flights of B quadrotors from hover, made once per batch size."""
    if B not in _SWARM:
        traj, lens = swarm_trajectories(11, 0, B)
        _SWARM[B] = (np.tile(traj[0, 0], (B, 1)), traj, lens)
    return _SWARM[B]


def flying_engine(lib, B, **cfg):
    x0, traj, lens = swarm(B)
    e = Engine(config(B, **cfg), lib_path=lib)
    e.set_trajectories(traj, lens)
    e.sim_reset(x0)
    return e


def whole(e):
    """Everything the cases compare: plant states, controls, trajectories, iterate, RGP mean and covariance, cursors, solver state and
    the tracking accumulators (snapshot) plus the reduced tracking statistic."""
    return dict(snapshot(e), tracking=e.get_tracking_stats())


_RUNS = {}


def closed_loop(lib, B, plants=None, groups=0, precision=0, period0=0):
    """K periods of sim_steps with `plants` (None: no fleet; 'defaults'; 'sample')."""
    key = (lib, B, plants, groups, precision, period0)
    if key not in _RUNS:
        e = flying_engine(lib, B, precision=precision, **(dict(tune=dict(groups=groups)) if groups else {}))
        if plants == "defaults":
            e.fleet_set(fleet_defaults(e.cfg, B), period0)
        elif plants == "sample":
            e.fleet_set(fleet_sample(5, 0, B, e.cfg, **SAMPLE), period0)
        e.sim_steps(K, NSUB, SIM_DT)
        _RUNS[key] = dict(whole=whole(e), groups=e.get_groups(), period=e.fleet_get()[1] if plants else None)
        e.close()
    return _RUNS[key]


# ------------------------------------------------------------------ 1. the reference's Quadrotor3D
def case_reference_vectors(lib, B):
    g, p = golden_plants(B)
    e = Engine(config(B), lib_path=lib)
    e.sim_reset(g["x0"][:B])
    e.fleet_set(p)
    assert e.sim_plant_period(g["u"][:B], CONTROL_DT, SIM_DT) == NSUB
    x, w = e.sim_get_state()
    assert e.fleet_get()[1] == 1 and np.array_equal(w, g["u"][:B])
    e.close()
    ref = g["x_ref"][:B]
    err = np.abs(x - ref)
    scaled = err / np.maximum(1.0, np.abs(ref))
    for name, sel in (("one_step_forward, disturbed", g["group"][:B] == 0), ("update, clipped inputs", g["group"][:B] == 1)):
        if sel.any():
            print(f"{name}: {int(sel.sum())} plants, worst deviation {err[sel].max():.3e} absolute, {scaled[sel].max():.3e} scaled")
    assert np.isfinite(x).all() and (scaled <= 1e-12).all(), scaled.max()
    # the extras are what moved the states: the engine's shared plant is far from every one of these
    e = Engine(config(B), lib_path=lib)
    e.sim_reset(g["x0"][:B])
    e.sim_plant_period(g["u"][:B], CONTROL_DT, SIM_DT)
    assert (np.abs(e.sim_get_state()[0] - ref).max(axis=1) > 1e-6).all()
    e.close()


# ------------------------------------------------------------------ 2. the oracle, one per quadrotor
def case_oracle_per_quadrotor(lib, B):
    from oracle.oracle import OracleEngine
    rng = np.random.default_rng(31)
    cfg = config(B)
    p = fleet_sample(7, 0, B, cfg, spread=2.0)           # mass, J, thrust, drag: what the oracle knows; geometry below
    for name in ("x_f", "y_f", "z_l_tau"):
        p[name] *= rng.uniform(0.5, 2.0, (B, 1))
    x0 = np.tile(swarm(1)[0], (B, 1))
    x0[:, 0:3] += rng.normal(0, 1.0, (B, 3))
    q = rng.normal(0, 0.25, (B, 4)) + np.array([1.0, 0, 0, 0])
    x0[:, 3:7] = q / np.linalg.norm(q, axis=1, keepdims=True)
    x0[:, 7:10], x0[:, 10:13] = rng.normal(0, 4.0, (B, 3)), rng.normal(0, 0.5, (B, 3))
    u = rng.uniform(-0.1, 1.1, (B, 4))
    e = Engine(cfg, lib_path=lib)
    e.sim_reset(x0)
    e.fleet_set(p)
    e.sim_plant_period(u, CONTROL_DT, SIM_DT)
    x = e.sim_get_state()[0]
    e.close()
    want = np.zeros_like(x)
    for b in range(B):
        quad = QuadParams(mass=p["mass"][b], J=p["J"][b], max_thrust=p["max_thrust"][b], x_f=p["x_f"][b], y_f=p["y_f"][b], z_l_tau=p["z_l_tau"][b],
                          g=cfg.quad.g, rotor_drag=p["rotor_drag"][b], aero_drag=p["aero_drag"][b])
        o = OracleEngine(EngineConfig(batch=1, N=10, T=1.0, quad=quad))
        want[b], n = o.plant_control_period(x0[b], u[b], CONTROL_DT, SIM_DT)
        assert n == NSUB
        o.close()
    scaled = np.abs(x - want) / np.maximum(1.0, np.abs(want))
    print(f"oracle per quadrotor: B = {B}, worst deviation {np.abs(x - want).max():.3e} absolute, {scaled.max():.3e} scaled")
    assert (scaled <= 1e-13).all(), scaled.max()
    assert len(np.unique(want[:, 9])) == B               # ... of B different plants


# ------------------------------------------------------------------ 3. default plants are the identity
def case_defaults_identity(lib, B, groupings=(0, 2), precision=0):
    for groups in groupings:                             # (0: the default grouping, one group at these sizes)
        plain, fleet = closed_loop(lib, B, groups=groups, precision=precision), closed_loop(lib, B, "defaults", groups=groups, precision=precision)
        assert plain["groups"] == fleet["groups"] == (groups or 1)
        print(f"default plants against no fleet, groups {groups or 1}, precision {precision}: largest difference plant state "
              f"{np.nanmax(np.abs(plain['whole']['x'] - fleet['whole']['x'])):.3e}, control {np.nanmax(np.abs(plain['whole']['w'] - fleet['whole']['w'])):.3e}")
        assert_same(plain["whole"], fleet["whole"])
        assert fleet["period"] == K
        assert np.isfinite(plain["whole"]["x"]).all() and (plain["whole"]["st_idx"] == K).all()


# ------------------------------------------------------------------ 4. group offsets with unequal plants
def case_group_offsets(lib, B):
    one, two, plain = closed_loop(lib, B, "sample"), closed_loop(lib, B, "sample", groups=2), closed_loop(lib, B, groups=2)
    assert one["groups"] == 1 and two["groups"] == 2
    assert_same(one["whole"], two["whole"])
    moved = np.abs(one["whole"]["x"] - plain["whole"]["x"]).max(axis=1)
    assert (moved > 1e-6).all()                          # every quadrotor flew a plant of its own
    assert len(np.unique(one["whole"]["x"][:, 2])) == B


# ------------------------------------------------------------------ 5. the disturbance window
def window_plants(cfg, B, window):
    p = fleet_sample(9, 0, B, cfg, spread=1.1, gust_force=1.0, gust_torque=0.02, gust_window=window)
    p["f_d"][1::2], p["t_d"][1::2] = 0.0, 0.0            # half the quadrotors feel it
    return p


def case_window(lib, B, groups=0):
    tune = dict(tune=dict(groups=groups)) if groups else {}
    for period0, periods, on in ((0, 7, range(2, 5)), (3, 3, range(3, 5))):
        e = flying_engine(lib, B, **tune)
        assert e.get_groups() == (groups or 1)
        e.fleet_set(window_plants(e.cfg, B, (2, 5)), period0)
        e.sim_steps(periods, NSUB, SIM_DT)
        assert e.fleet_get()[1] == period0 + periods     # the fleet period counts periods, not launches
        got = whole(e)
        e.close()
        # the host loop: the window is the host's, one table per period
        h = flying_engine(lib, B, **tune)
        h.fleet_set(window_plants(h.cfg, B, (0, 0)), period0)
        for k in range(periods):
            p = period0 + k
            h.fleet_set(window_plants(h.cfg, B, (INT_MIN, INT_MAX) if p in on else (0, 0)), -1)
            assert h.fleet_get()[1] == p
            w, _ = h.step(h.sim_get_state()[0])
            h.sim_plant_period(w, CONTROL_DT, SIM_DT)
        assert h.fleet_get()[1] == period0 + periods
        want = whole(h)
        h.close()
        assert_same(want, got)
    # ... and the window acts: a plant update inside it moves the disturbed half elsewhere than one outside it, the other half not
    ends = []
    for period0 in (1, 2, 4, 5):
        e = Engine(config(B), lib_path=lib)
        e.sim_reset(swarm(B)[0])
        e.fleet_set(window_plants(e.cfg, B, (2, 5)), period0)
        e.sim_plant_period(np.full((B, 4), 0.3), CONTROL_DT, SIM_DT)
        ends.append(e.sim_get_state()[0])
        e.close()
    assert np.array_equal(ends[1], ends[2]) and np.array_equal(ends[0], ends[3])
    d = np.abs(ends[1] - ends[0]).max(axis=1)
    assert (d[0::2] > 1e-6).all() and (d[1::2] == 0).all()


# ------------------------------------------------------------------ 6. under a mission, with recorder and score running
REC_FIELDS = ("x_odom", "x_ref", "w_odom", "cost_solution", "solver")


KM = 4   # periods of the mission case: the flights are installed behind period 0


def mission_run(lib, B, blocks, fleet=True):
    L, Tmax = 2, 300
    rng = np.random.default_rng(41)
    x0, traj, lens = hover_slots(B, Tmax, 43)
    wp = x0[:, None, None, 0:3] + rng.uniform(-0.5, 0.5, (B, L, 2, 3))
    e = Engine(config(B), lib_path=lib)
    e.set_trajectories(traj, lens)
    e.sim_reset(x0)
    if fleet:
        e.fleet_set(fleet_sample(13, 0, B, e.cfg, **SAMPLE))
    e.mission_set(wp, 5.0, 10.0, dt=DT)
    e.score_start(3)
    e.record_start(fields=REC_FIELDS, every=1, capacity=KM)
    x_hist = []
    for n in blocks:
        e.sim_steps(n, NSUB, SIM_DT)
        x_hist.append(e.sim_get_state()[0])
    run = dict(whole=whole(e), rec=e.record_get(), mission=e.mission_get(), score=e.score_get(), x_hist=x_hist)
    e.close()
    return run


def case_mission(lib, B):
    # (the run without a fleet is only asked where its quadrotors stand at the start of period 1: two periods are enough)
    one, each, plain = mission_run(lib, B, [KM]), mission_run(lib, B, [1] * KM), mission_run(lib, B, [2], fleet=False)
    assert_same(one["whole"], each["whole"])
    assert_same(one["rec"], each["rec"], [k for k in one["rec"] if k != "dropped"])
    assert_same(one["mission"], each["mission"], ("leg", "installed", "leg_code", "leg_period"))
    assert_same(one["score"], each["score"])
    ms = each["mission"]
    assert (ms["leg_period"][:, 0] == 0).all() and (ms["leg_code"][:, 0] == 0).all() and (ms["installed"] >= 1).all()
    # plant in front of mission: the first flight starts where the FLEET plant stood behind the update of period 0 (rows are rounded to
    # 6 decimals), which is not where the shared plant stood
    start = each["rec"]["x_ref"][:, 1, 0:3]              # row 0 of the chunk period 1 used: the first row of the new flight
    assert np.abs(start - each["x_hist"][0][:, 0:3]).max() <= 0.5e-6 + 1e-12
    assert (np.abs(plain["rec"]["x_odom"][:, 1] - each["rec"]["x_odom"][:, 1]).max(axis=1) > 1e-6).all()


# ------------------------------------------------------------------ 7. refusals and stop
def case_rules(lib, B=8):
    x0, traj, lens = swarm(B)
    e = flying_engine(lib, B)
    assert b"mpcq 0.6.7" in e.lib.mpcq_version()
    size = PLANT_DTYPE.itemsize
    for fn in (lambda: e.lib.mpcq_fleet_get(e.h, None, size, None), lambda: e.lib.mpcq_fleet_stop(e.h)):
        assert fn() == MPCQ_ERR_STATE                                # no fleet set
    good = fleet_sample(17, 0, B, e.cfg, **SAMPLE)
    e.sim_steps(1, NSUB, SIM_DT)

    def refused(p, *names, plant_size=size, period0=0):
        before = whole(e)
        table = e.fleet_get() if e.lib.mpcq_fleet_get(e.h, None, size, None) == 0 else None
        assert e.lib.mpcq_fleet_set(e.h, p.ctypes.data_as(_lib._vp), plant_size, period0) == MPCQ_ERR_INVALID
        msg = e.lib.mpcq_last_error().decode()
        for n in names:
            assert n in msg, (n, msg)
        assert_same(before, whole(e))
        if table is None:
            assert e.lib.mpcq_fleet_stop(e.h) == MPCQ_ERR_STATE      # the refused call set no fleet
        else:
            now = e.fleet_get()
            assert now[0].tobytes() == table[0].tobytes() and now[1] == table[1]

    def bad_tables():
        yield good, ("plant_size",), dict(plant_size=size - 8)
        yield good, ("plant_size",), dict(plant_size=size + 8)
        yield good, ("period0",), dict(period0=-2)
        for name in PLANT_DTYPE.names[:-2]:
            for v in (np.nan, np.inf):
                p = good.copy()
                b = B - 1 if name == "mass" else 2
                if p[name].ndim > 1:
                    p[name][b, 1] = v
                    yield p, (f"quadrotor {b}", f"{name}[1]", "finite"), {}
                else:
                    p[name][b] = v
                    yield p, (f"quadrotor {b}", name, "finite"), {}
        for name, v in (("mass", 0.0), ("mass", -1.0), ("max_thrust", 0.0)):
            p = good.copy()
            p[name][3] = v
            yield p, ("quadrotor 3", name, "> 0"), {}
        p = good.copy()
        p["J"][4, 2] = 0.0
        yield p, ("quadrotor 4", "J[2]", "> 0"), {}
        for v in (-1e-9, 1.0 + 1e-9):
            p = good.copy()
            p["rotor_functionality"][5, 3] = v
            yield p, ("quadrotor 5", "rotor_functionality[3]", "[0, 1]"), {}

    tables = list(bad_tables())
    for p, names, kw in tables[:6]:                                   # with no fleet set ...
        refused(p, *names, **kw)
    e.fleet_set(good, period0=5)
    for p, names, kw in tables:                                       # ... and with one
        refused(p, *names, **kw)
    got, period = e.fleet_get()
    assert got.tobytes() == good.tobytes() and period == 5            # the table round-trips exactly
    expect_rc(MPCQ_ERR_STATE, e.sim_run, 2, NSUB, SIM_DT)             # one persistent launch with the shared plant fused in
    assert "fleet" in e.lib.mpcq_last_error().decode()
    e.sim_steps(2, NSUB, SIM_DT)
    e.reset()                                                         # keeps the table and the period
    got, period = e.fleet_get()
    assert got.tobytes() == good.tobytes() and period == 7
    e.set_trajectories(traj, lens)
    e.sim_steps(2, NSUB, SIM_DT)
    edge = good.copy()                                                # the closed ends of the ranges are legal
    edge["rotor_functionality"][0], edge["payload_mass"][1], edge["d_from"][2], edge["d_to"][2] = (0.0, 1.0, 1.0, 0.0), 0.0, INT_MIN, INT_MAX
    e.fleet_set(edge, period0=-1)
    assert e.fleet_get()[1] == 9
    e.fleet_set(good, period0=-1)
    # after fleet_stop: the periods of an engine that never had a fleet and stands where this one stands
    n = Engine(config(B), lib_path=lib)
    n.set_trajectories(traj, lens)
    n.set_state(**e.get_state())
    n.set_solver_state(**e.get_solver_state())
    n.sim_reset(e.sim_get_state()[0])
    e.fleet_stop()
    expect_rc(MPCQ_ERR_STATE, e.fleet_stop)
    expect_rc(MPCQ_ERR_STATE, e.fleet_get)
    for eng in (e, n):
        eng.sim_steps(3, NSUB, SIM_DT)
    assert_same(whole(n), whole(e))
    e.sim_run(1, NSUB, SIM_DT)                                        # legal again
    e.fleet_set(good, period0=-1)                                     # -1 with none active: 0
    assert e.fleet_get()[1] == 0
    e.close(); n.close()


# ------------------------------------------------------------------ 8. CPU only
def header_struct(name):
    """[(field, ctype, count)] of `typedef struct <name> { ... }` in include/mpcq.h."""
    with open(os.path.join(HERE, "..", "include", "mpcq.h")) as fh:
        text = re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, flags=re.S).group(1)
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ctype, rest = decl.split(None, 1)
        for item in rest.split(","):
            m = re.fullmatch(r"\s*(\w+)\s*(?:\[(\d+)\])?\s*", item)
            out.append((m.group(1), ctype, int(m.group(2) or 1)))
    return out


def test_plant_dtype_matches_header():
    sizes = {"double": (8, np.float64), "int32_t": (4, np.int32)}
    fields = header_struct("mpcq_plant")
    assert [f[0] for f in fields] == list(PLANT_DTYPE.names)
    off = align = 0
    for name, ctype, count in fields:
        size, dt = sizes[ctype]
        off = -(-off // size) * size
        sub = PLANT_DTYPE.fields[name]
        assert sub[1] == off and sub[0].base == dt and sub[0].shape == (() if count == 1 else (count,)), name
        off += size * count
        align = max(align, size)
    assert PLANT_DTYPE.itemsize == -(-off // align) * align == 264


def test_fleet_sample_shards_agree():
    cfg = config(16)
    a, b = fleet_sample(3, 0, 16, cfg, **SAMPLE), fleet_sample(3, 8, 8, cfg, **SAMPLE)
    assert a[8:].tobytes() == b.tobytes()
    d = fleet_defaults(cfg, 16)
    assert (a["mass"] != d["mass"]).all() and len(np.unique(a["mass"])) == 16 and (a["rotor_functionality"] < 1).any()
    assert (a["rotor_functionality"] >= SAMPLE["fault_min"]).all() and (a["payload_mass"] <= SAMPLE["payload_max"]).all()
    assert (np.abs(np.log(a["mass"] / d["mass"])) <= np.log(SAMPLE["spread"]) + 1e-12).all()
    assert (a["d_from"] == 1).all() and (a["d_to"] == 4).all()
    same = fleet_sample(3, 0, 16, cfg.quad, spread=1.0)              # nothing asked for: the defaults
    assert same.tobytes() == d.tobytes()
    q = cfg.quad
    assert d["mass"][0] == q.mass and tuple(d["J"][0]) == tuple(q.J) and tuple(d["z_l_tau"][0]) == tuple(q.z_l_tau)
    assert (d["rotor_functionality"] == 1).all() and (d["payload_mass"] == 0).all() and (d["f_d"] == 0).all() and (d["d_to"] == 0).all()


def test_contraction_matches_plant_kernel():
    """The GPU identity of default plants (case 3) needs fleet_plant_kernel to fuse plant_eval's multiplications and additions exactly as
    plant_kernel does (csrc/mpcq_fleet.hpp).  tools/fleet_contraction_check.py reads that off the disassembly of the built object: no GPU.
    Skips where the object or the disassembler is not there (the object is a build product)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("fleet_contraction_check", os.path.join(HERE, "..", "tools", "fleet_contraction_check.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    if not os.path.exists(tool.DEFAULT_OBJ) or not all(os.path.exists(os.path.join(tool.LLVM, t)) for t in ("llvm-objdump", "llvm-objcopy", "clang-offload-bundler")):
        pytest.skip("no built csrc/build/api.o, or no llvm-objdump / llvm-objcopy / clang-offload-bundler")
    missing, report = tool.check(tool.DEFAULT_OBJ)
    print(report)
    assert not missing, missing


def test_drag_truth_matches_reference():
    g, p = golden_plants(128)
    assert np.array_equal(fleet_drag_accel(p, g["drag_v"]), g["drag_a"])
    one = fleet_drag_accel(p, g["drag_v"][5, 0])                     # one grid for every axis and plant
    assert one.shape == (128, 3, 6) and np.array_equal(one[5, 0], g["drag_a"][5, 0])


# ------------------------------------------------------------------ lane emulator (CPU)
def test_emu_reference_vectors(emu):
    case_reference_vectors(emu, 16)


def test_emu_oracle_per_quadrotor(emu):
    case_oracle_per_quadrotor(emu, 16)


def test_emu_defaults_identity(emu):
    case_defaults_identity(emu, 16, groupings=(2,))


def test_emu_group_offsets(emu):
    case_group_offsets(emu, 16)


def test_emu_window(emu):
    case_window(emu, 8)
    case_window(emu, 16, groups=2)


def test_emu_mission(emu):
    case_mission(emu, 8)


def test_emu_rules(emu):
    case_rules(emu)


# ------------------------------------------------------------------ MI355X
gpu = pytest.mark.gpu


@gpu
def test_gpu_reference_vectors():
    case_reference_vectors(None, 128)


@gpu
def test_gpu_oracle_per_quadrotor():
    case_oracle_per_quadrotor(None, 70)


@gpu
@pytest.mark.parametrize("precision", [0, 1])
def test_gpu_defaults_identity(precision):
    case_defaults_identity(None, 70, precision=precision)


@gpu
def test_gpu_group_offsets():
    case_group_offsets(None, 70)


@gpu
def test_gpu_window():
    case_window(None, 70)
    case_window(None, 70, groups=2)


@gpu
def test_gpu_mission():
    case_mission(None, 70)


@gpu
def test_gpu_rules():
    case_rules(None, B=70)


@gpu
def test_gpu_drag_truth_through_engine():
    """Engine.fleet_drag_truth reads the table back from the engine."""
    g, p = golden_plants(128)
    e = Engine(config(128))
    e.fleet_set(p)
    assert np.array_equal(e.fleet_drag_truth(g["drag_v"]), g["drag_a"])
    e.close()

"""The float interior point of the fp64 fallback solve on four-stage blocks (mpcq_kernels.hpp: blk_form, blk_factor, blk_forward,
blk_backward_vec; -DMPCQ_BLOCK_IPM, default 1) against the stage-wise iteration (-DMPCQ_BLOCK_IPM=0) and against the fp64 oracle.
The interior point only names a working set: the answer of every solve comes from the double active-set method behind it, so the two
builds must end on the same optimum, and the block build must not hand over a worse guess (more passes behind it).

CPU: both builds of the shape-specialised (20, 10) instance on the lane emulator (tests/wave_emu), compiled here into a temporary
directory the way the Makefile's `brk` recipe does.  GPU: the product library at (20, 10) and (20, 20) in the three layouts."""
import os
import subprocess

import numpy as np
import pytest

import parity_cases as pc
from helpers import GOLDEN  # noqa: F401  (tests/helpers.py is the suite's shared module)
from mpc_quad_ros_amd.engine import Engine, qp_fallback, qp_flip
from mpc_quad_ros_amd.params import EngineConfig, hummingbird, rgp_basis_linspace

EMU_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "wave_emu")
EMU = os.path.join(EMU_DIR, "libmpcq_emu.so")
SRC = os.path.join(os.path.dirname(EMU_DIR), os.pardir, "mpc_quad_ros_amd", "csrc")
CXX = "/opt/rocm/lib/llvm/bin/clang++"
CXXFLAGS = ["-O2", "-g", "-DMPCQ_EMU_BUILD", "-fno-strict-aliasing", "-std=c++17", "-fPIC", "-I" + EMU_DIR, "-x", "c++", "-Wno-unknown-pragmas",
            "-Wno-pass-failed", "-Wno-unused-command-line-argument", "-w"]
EPS = np.finfo(np.float64).eps


def emu_variant(tmp, name, define):
    """libmpcq_emu.so with the (20, 10) instance recompiled with `define` (the other objects are the emulator's own)."""
    subprocess.check_call(["make", "-C", EMU_DIR], stdout=subprocess.DEVNULL)
    obj, lib = os.path.join(tmp, f"spec_20_10_{name}.o"), os.path.join(tmp, f"libmpcq_emu_{name}.so")
    subprocess.check_call([CXX, *CXXFLAGS, define, "-DMPCQ_SPEC_N=20", "-DMPCQ_SPEC_NB=10", "-c", "-o", obj, os.path.join(SRC, "mpcq_spec.hip")])
    others = [os.path.join(EMU_DIR, "obj", f) for f in ("rt.o", "api.o", "learn.o", "spec_20_20.o", "spec_50_50.o")]
    subprocess.check_call([CXX, "-shared", "-o", lib, *others, obj, "-ldl"])
    return lib


def recording(lib, log):
    """make_engine of parity_cases whose engine notes, per step: controls, status, qp_iter, factorisations, float iterations, breakdowns
    (bit 15 of the work word)."""
    def make(cfg):
        e = Engine(cfg, lib_path=lib)
        step = e.step
        def step_and_record(x):
            out = step(x)
            log.append(dict(w=np.array(out[0]), status=e.get_status().copy(), it=e.get_qp_iter().copy(), work=e.get_qp_work()[0].copy(),
                            fit=e.get_qp_float_iterations().copy(), brk=e.get_qp_float_breakdown().copy()))
            return out
        e.step = step_and_record
        return e
    return make


def stack(log, key):
    return np.stack([r[key] for r in log])


@pytest.fixture(scope="module")
def emu_runs(tmp_path_factory):
    """The saturating-reference closed loop of parity_cases at (20, 10), B = 4, a cold start + 5 periods, on both emulator builds."""
    tmp = str(tmp_path_factory.mktemp("block_ipm"))
    stage = emu_variant(tmp, "stagewise", "-DMPCQ_BLOCK_IPM=0")
    runs = {}
    for name, lib in (("block", EMU), ("stage", stage)):
        log = []
        worst, hist, failed = pc.case_saturating_references(recording(lib, log), B=4, K=6)
        runs[name] = dict(log=log, worst=worst, hist=hist, failed=failed)
    return runs


def test_emu_block_and_stagewise_builds_end_on_the_same_optimum(emu_runs):
    for name, r in emu_runs.items():
        st, it = stack(r["log"], "status"), stack(r["log"], "it")
        print(name, "worst deviation vs oracle", r["worst"], "qp_iter", dict(sorted(r["hist"].items())))
        assert (st == 0).all() and r["failed"] == 0, (name, st)
        assert r["worst"] < 1e-7, (name, r["worst"])                       # the budget of test_emu_saturating_references_many_working_sets
        assert not stack(r["log"], "brk").any()
        assert qp_fallback(it).sum() >= 10 and qp_flip(it).sum() >= 3, (name, it)   # the fixture holds fallback solves, flip-marked ones among them
        assert (stack(r["log"], "fit")[0] >= 2).all()                          # the cold start went through the float interior point
    wb, ws = stack(emu_runs["block"]["log"], "w"), stack(emu_runs["stage"]["log"], "w")
    diff, scale = np.abs(wb - ws).max(), np.abs(ws).max()
    print("controls block vs stage-wise: max difference", diff, "largest control", scale, "bound", 64 * EPS * scale)
    assert diff <= 64 * EPS * scale                                          # the polish's own multiplier tolerance


def test_emu_block_build_hands_over_no_worse_working_sets(emu_runs):
    """Factorisations that are not float interior-point iterations (warm attempt, which both builds run on the same data, + the active-set
    passes behind the interior point), summed over the fallback solves: at most one more per fallback solve on the block build."""
    tot = {}
    for name, r in emu_runs.items():
        it, work, fit = stack(r["log"], "it"), stack(r["log"], "work"), stack(r["log"], "fit")
        fb = qp_fallback(it)
        tot[name] = (int((work - fit)[fb].sum()), int(fb.sum()), int(fit[fb].sum()))
    print("(passes, fallback solves, float iterations) by build:", tot)
    assert tot["block"][1] == tot["stage"][1] >= 10
    assert tot["block"][0] - tot["stage"][0] <= tot["block"][1]


def test_emu_block_interior_point_breakdown_recovers(tmp_path):
    """Negative hand-over tolerance with the block path on: every float stage breaks down (a non-positive pivot of a block Hessian) or
    hits its cap, and the solve recovers through the double interior point with bit 15 of the work word set."""
    brk = emu_variant(str(tmp_path), "blkbrk", "-DMPCQ_HYBRID_TOL=-1.0f")
    log = []
    worst, hist, failed = pc.case_saturating_references(recording(brk, log), B=2, K=4)
    it, bd = stack(log, "it"), stack(log, "brk")
    fb = qp_fallback(it)
    print("block breakdown build: worst", worst, "fallback solves", int(fb.sum()), "breakdowns", int(bd.sum()))
    assert failed == 0 and worst < 1e-7
    assert fb.sum() >= 2 and bd[fb].all() and bd[0].all()


def saturating_trajectories(B, T):
    """The references of parity_cases.case_saturating_references (fast lateral sinusoid + vertical steps)."""
    traj = np.zeros((B, T, 13)); traj[:, :, 3] = 1.0
    t = np.arange(T) * 0.01
    for b in range(B):
        A, w = 2.0 + b, 3.0 + 0.7 * b
        traj[b, :, 0] = A * np.sin(w * t); traj[b, :, 7] = A * w * np.cos(w * t)
        traj[b, :, 2] = 3.0 + 1.5 * np.sign(np.sin(2.0 * t + b))
    return traj, np.full(B, T, dtype=np.int32)


@pytest.mark.gpu
@pytest.mark.parametrize("nb", [10, 20])
@pytest.mark.parametrize("mem", [1, 2, 3])
def test_gpu_block_interior_point_in_every_layout(nb, mem):
    B, N, K = 8, 20, 31
    tune = dict(stage_mem=mem)
    log = []
    worst, hist, failed = pc.case_saturating_references(recording(None, log), B=B, K=K, N=N, nb=nb, tune=tune)
    it = stack(log, "it")
    print(f"N={N} nb={nb} layout {mem}: worst {worst:.2e} failed {failed} fallback solves {int(qp_fallback(it).sum())} "
          f"float iterations on the cold start {log[0]['fit']}")
    assert failed == 0 and worst < pc.TOL_TF[0]
    assert (log[0]["fit"] >= 2).all()
    assert not stack(log, "brk").any()
    assert qp_fallback(it).sum() >= 10
    # lockstep launches against the free-running launch on the same references, bit for bit
    traj, lens = saturating_trajectories(B, 60 + K * 5)
    x0 = np.tile(np.array([0, 0, 3.0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0]), (B, 1))
    out = []
    for mode in ("sim_steps", "sim_run"):
        e = Engine(EngineConfig(batch=B, N=N, quad=hummingbird(), nb=nb, basis=rgp_basis_linspace(12.0, nb), tune=tune))
        e.set_trajectories(traj, lens); e.sim_reset(x0)
        getattr(e, mode)(K, 2, 5e-3)
        out.append((*e.sim_get_state(), e.get_state()["X"], e.get_state()["U"], e.get_qp_iter()))
        e.close()
    for a, b in zip(*out):
        assert np.array_equal(a, b)

"""The step kernel against the fp64 CPU oracle at the shapes where its index arithmetic changes, on every working-set layout.

mpcq_create accepts 2 <= N <= 128 and 0 <= nb <= 128 and picks one of three working-set layouts; the other suites run N in {5, 10, 20, 50}
with nb in {0, 10, 20, 50} and the layout the selection rule picks.  Every shape of SHAPES sits on one edge of the kernel (the table
there), and every cell runs the any-shape instance (Cfg<T, GAB, 0, -1, RUN, GK>: none of the shapes has a specialised one):

  1. shape matrix: SHAPES x both precisions x tune.stage_mem 1 / 2 / 3, B = 4: case_explicit_api and 6 periods of case_swarm_closed_loop.
     A forced layout that does not fit 160 KiB of LDS has to be refused by create with MPCQ_ERR_INVALID and a message naming the limit;
     whether it fits is computed here, in numpy, from the documented layout (host_lds_bytes), never asked of the library.  Plus the
     largest accepted corner, N = 128 with nb = 128 and nb = 0, layout left to the engine.
     And the GP term with a basis dense enough that every basis point counts (_every_basis_point: N = 2, nb on both sides of the unroll).
  2. saturated working sets (case_saturating_references) at the tile and row edges: restarted factorisations, fallbacks.
  3. (tests/test_gpu_parity.py, tests/test_engine_edges.py: free-running == lockstep at (3,7), (17,10), (33,65).)
  4. groups and cost-sorted block order at batches that are no multiple of the 8-quadrotor granule (B = 13: one group, B = 21: 16 + 5).

Two layers over the same case functions, as in the other case files: test_emu_* on the lane emulator (tests/wave_emu: the product kernel
sources compiled for the host; lane logic, LDS layout, barriers) and test_gpu_* (marked gpu) on libmpcq.so.  Emulator time grows steeply
with N, so the split is:
  * emulator: the matrix for N <= 17 (all three layouts, both precisions) plus (21,33) on layout 0 in fp64; the saturated runs on layout 0
    and the compact layout; the dense-basis and the groups case; of the 128 corner the shapes create has to refuse (no kernel runs).
  * GPU: every cell, i.e. also (24,9), (33,65), (64,3) and the corner shape that fits (N = 128, nb = 0).
No cell is skipped: a cell either runs or asserts the refusal the host-side formula predicts."""
import dataclasses
import os
import subprocess

import numpy as np
import pytest

import parity_cases as pc
from mpc_quad_ros_amd import _lib
from mpc_quad_ros_amd.engine import Engine, qp_fallback, qp_passes
from mpc_quad_ros_amd.params import EngineConfig, hummingbird, rgp_basis_linspace
from mpc_quad_ros_amd.trajectories import swarm_trajectories

EMU_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "wave_emu")
EMU = os.path.join(EMU_DIR, "libmpcq_emu.so")

#          N   nb    the edge
SHAPES = [(2, 0),    # minimum horizon, no GP
          (2, 1),    # minimum of both
          (3, 7),    # a single cost-to-go tile, a restart rounds past the horizon end; nb below the unroll of alpha = Kx^-1 mu
          (4, 64),   # the RGP workspace decides the size of the union region; 3 nb = 192: exactly three lane rows
          (5, 22),   # 3 nb = 66: two lanes into a second row; unroll remainder 2
          (7, 13),   # N = 4k + 3
          (16, 12),  # nv = 4 N = 64: exactly one register row
          (17, 10),  # first partial second row
          (21, 33),  # first N > 20 (abort_pins / abort_wrong defaults change formula)
          (24, 9),   # first keep_ref false ((N + 1) 13 > 320)
          (33, 65),  # nb > 64
          (64, 3)]   # nv = 256
LAYOUTS = {1: "lds", 2: "global", 3: "compact"}      # tune.stage_mem -> layout 0 / 1 / 2 of lds_layout
LDS_LIMIT = 160 * 1024
LIMIT_MESSAGES = ("per-instance working set exceeds 160 KiB LDS with the stage records in LDS (tune.stage_mem = 1)",
                  "per-instance working set exceeds 160 KiB LDS (N/nb too large for this precision)")


def host_lds_bytes(N, nb, layout, precision):
    """LDS bytes of one quadrotor's working set (the documented layout restated, not read from the library).
    A double block -- iterate X [(N+1) 13], U [4N], x0 + post scratch [21], the prefetched persistent state [18]; mixed precision: the QP
    solution in double [4N] -- and a block of TQ elements (8 bytes in fp64, 4 in f32).  Every array is rounded up to 4 elements.
    layout 0 keeps the stage records AB'' [N 13 16 + 16], c [16 N], q [16 (N+1)] in LDS; layouts 1 and 2 keep a zero block [16] and the
    exchange scratch [22 x 8] instead.  Then alpha and the basis [3 nb each], the weights [48], mixed precision: the curvatures [4N].
    Behind them the union region, the largest of: shooting records [N (4 x 31 + 1)] | QP workspace: 13 input-sized vectors [4N] (r0, lb, ub and
    ten more; in the compact layout r0 / lb / ub live here too, so the count is the same), grad and vin [16 N], dx and Dx [16 (N+1)], the
    Riccati gains K [64 N] and Lambda^-1 [16 N] (layouts 0 and 1 only), three small tiles [64, 64, 32] | RGP workspace [3 nb^2 + 5 x 3 nb + 32]."""
    al4 = lambda v: (v + 3) & ~3
    mixed = precision == 1
    nv = 4 * N
    d = al4((N + 1) * 13) + al4(nv) + al4(21) + al4(18) + (al4(nv) if mixed else 0)
    q = (al4(N * 208 + 16) + al4(16 * N) + al4(16 * (N + 1))) if layout == 0 else (16 + 176)
    q += 2 * al4(3 * nb) + 48 + (nv if mixed else 0)
    outside = 0 if layout == 2 else 3 * nv                      # r0 / lb / ub in front of the union (layouts 0, 1) or inside it (compact)
    qp = (13 * nv - outside) + 2 * 16 * N + 2 * 16 * (N + 1) + (0 if layout == 2 else 64 * N + 16 * N) + 64 + 64 + 32
    union = max(al4(N * 125), qp, al4(3 * nb * nb) + 5 * al4(3 * nb) + 32)
    return 8 * d + (q + outside + union) * (4 if mixed else 8)


def fits(N, nb, stage_mem, precision):
    return host_lds_bytes(N, nb, stage_mem - 1, precision) <= LDS_LIMIT


def test_host_lds_formula_reproduces_the_documented_sizes():
    """host_lds_bytes against the figures of DESIGN.md section 3.1 (N = 20, nb = 10, all six; N = 50, nb = 50: fp64 compact 78.0 KB, f32
    layout 1 51.8 KB), and what it predicts for the cells below: which forced layouts of the matrix create has to refuse, and that of
    the 128 corner nb = 128 fits nowhere while nb = 0 fits (in fp64 only in the compact layout)."""
    assert [host_lds_bytes(20, 10, l, p) for p in (0, 1) for l in (0, 1, 2)] == [75648, 38528, 25728, 40384, 21824, 15424]
    assert host_lds_bytes(50, 50, 2, 0) == 77952 and host_lds_bytes(50, 50, 1, 1) == 51808
    assert host_lds_bytes(50, 50, 0, 0) > LDS_LIMIT                          # (tests/test_gpu_parity.py: test_kernel_variants_agree)
    refused = sorted((N, nb, sm, p) for N, nb in SHAPES for p in (0, 1) for sm in LAYOUTS if not fits(N, nb, sm, p))
    assert refused == [(33, 65, 1, 0), (64, 3, 1, 0)], refused
    assert not any(fits(128, 128, sm, p) for sm in LAYOUTS for p in (0, 1))
    assert [fits(128, 0, sm, 0) for sm in LAYOUTS] == [False, False, True] and [fits(128, 0, sm, 1) for sm in LAYOUTS] == [False, True, True]


# ------------------------------------------------------------------ cases (lib: None = the product library, else the emulator's)

def _maker(lib, **tune):
    return lambda cfg: Engine(dataclasses.replace(cfg, tune=dict(cfg.tune or {}, **tune)) if tune else cfg, lib_path=lib)


def _config(B, N, nb, precision, tune=None, skip=None):
    return EngineConfig(batch=B, N=N, quad=hummingbird(), nb=nb, basis=rgp_basis_linspace(12.0, nb) if nb else None, precision=precision,
                        tune=tune, skip=skip)


def _assert_refused(lib, N, nb, precision, tune, skip=None):
    with pytest.raises(_lib.MpcqError) as ex:
        Engine(_config(2, N, nb, precision, tune, skip), lib_path=lib)
    msg = str(ex.value)
    assert msg.startswith("mpcq error -1:") and any(m in msg for m in LIMIT_MESSAGES), msg      # MPCQ_ERR_INVALID, naming the limit


def _matrix_cell(lib, N, nb, precision, stage_mem, B=4, skip=None):
    """One cell of the matrix.  Returns the worst per-quadrotor control deviation of the closed loop, or None where the forced layout
    does not fit and create refused it as predicted."""
    tune = dict(stage_mem=stage_mem) if stage_mem else None
    if stage_mem and not fits(N, nb, stage_mem, precision):
        _assert_refused(lib, N, nb, precision, tune, skip)
        return None
    make = _maker(lib, **(tune or {}))
    pc.case_explicit_api(make, B=B, N=N, nb=nb, precision=precision, skip=skip)
    return pc.case_swarm_closed_loop(make, B=B, N=N, nb=nb, K=6, precision=precision, skip=skip)


def _matrix_shape(lib, N, nb, precision, layouts=(1, 2, 3)):
    for sm in layouts:
        worst = _matrix_cell(lib, N, nb, precision, sm)
        if worst is None:
            print(f"shape sweep N={N} nb={nb} layout {LAYOUTS[sm]} precision {precision}: refused by create (over 160 KiB), as predicted")
            continue
        print(f"shape sweep N={N} nb={nb} layout {LAYOUTS[sm]} precision {precision}: worst deviation {worst:.2e}")
        # the bounds of this case elsewhere: fp64 1e-7 (test_emu_swarm_closed_loop_hummingbird), f32 the 1e-4 budget (TOL_TF)
        assert worst < pc.TOL_TF[precision], (N, nb, LAYOUTS[sm], precision, worst)


def _corner(lib, nb, precision):
    """N = 128 (skip = 1: the node's int((T / N) / 0.01) is 0 there), layout left to the engine: it takes one that fits if there is one
    (the all-LDS one, else layout 1, else the compact one), so create refuses exactly when none of the three fits."""
    N = 128
    if not any(fits(N, nb, sm, precision) for sm in LAYOUTS):
        _assert_refused(lib, N, nb, precision, None, skip=1)
        return None
    worst = _matrix_cell(lib, N, nb, precision, 0, B=2, skip=1)
    print(f"shape sweep N={N} nb={nb} precision {precision}: worst deviation {worst:.2e}")
    assert worst < pc.TOL_TF[precision], (nb, precision, worst)
    return worst


def _every_basis_point(lib, nb, precision):
    """The GP term with every basis point in play.  The node's basis spans +-12 m/s at unit length scale: at the velocities of the cases above
    only the points next to 0 contribute, K_x is all but diagonal, and an element of mu or a row of alpha = Kx^-1 mu at the far end of the
    basis moves the controls by 1e-13 (measured on the emulator: the remainder loop of alpha one element short passes every cell of the
    matrix).  Here the basis spans +-2 m/s, inside the +-1.2 m/s the states of case_explicit_api fly at: K_x is dense, every element of
    alpha depends on every element of mu and every basis point on the prediction.  N = 2, the cheapest horizon; nb on both sides of the
    unroll by 5 and of the 64-lane rows of 3 nb and 3 nb^2."""
    pc.case_explicit_api(_maker(lib), B=3, N=2, nb=nb, precision=precision, basis_vmax=2.0)


BASIS_SIZES = [1, 4, 7, 13, 22, 33, 64, 65]


SATURATED = [(3, 7), (7, 13), (16, 12), (17, 10), (21, 33)]
# Factor on the references' amplitude per shape (parity_cases.case_saturating_references `amplitude`).  The references were made for a
# 1 s horizon of 20 stages; every shape here runs them unscaled (checked on the emulator and the oracle: fallbacks and many-pass solves at
# every shape, see _saturated).
AMPLITUDE = {}


def _saturated(lib, N, nb, precision, stage_mem, K):
    worst, hist, failed = pc.case_saturating_references(_maker(lib), B=3, K=K, precision=precision, N=N, nb=nb, tune=dict(stage_mem=stage_mem),
                                                        amplitude=AMPLITUDE.get((N, nb), 1.0))
    print(f"saturating references N={N} nb={nb} layout {LAYOUTS[stage_mem]} precision {precision}: worst {worst:.2e} failed {failed} passes",
          dict(sorted(hist.items())))
    assert failed == 0
    assert worst < (1e-7 if precision == 0 else pc.TOL_TF[1])
    # not vacuous: the run has a solve that went through more than one working set, and a fallback solve.  N = 3 is the exception to the
    # second: its QP has 12 inputs.  Over the first 17 periods both sides (oracle and engine agree to 4e-12) put 276 of the 612 horizon inputs
    # of the 51 solves at a bound and the warm attempt goes through up to 11 working sets (13 in f32) -- but never gives up, the cold start
    # included: below abort_pins = 10 first-pass pins and inside warm_max = 12 passes there is nothing to fall back from (the 40-period run
    # has four fallbacks behind period 17).  What is asserted there is the many-pass warm attempt.
    assert any(qp_passes(v) > 1 and not qp_fallback(v) for v in hist), hist
    if N == 3:
        assert max(int(qp_passes(v)) for v in hist if not qp_fallback(v)) >= 5, hist
    else:
        assert any(qp_fallback(v) for v in hist), hist


def _groups_odd_batch(lib, B, split):
    """tune.groups = 2 with the cost-sorted launch order at a batch that is no multiple of the 8-quadrotor granule, N = 7, nb = 13, 6 periods of
    sim_steps: bit for bit the run of one group in index order -- plant state, controls, iterate, RGP posterior, cursors, tracking statistic.
    A group takes ((B + 1) / 2 + 7) / 8 * 8 quadrotors and the last one what is left, but a group holds at least one quadrotor of every
    launch-order class (B / groups >= 8, mpcq_api.hip init): B = 13 is therefore run as ONE group of 13 whatever tune.groups asks for
    (split = (13,)); B = 21 is the smallest odd batch that is cut, into 16 + 5 (split = (16, 5))."""
    N, nb = 7, 13
    traj, lens = swarm_trajectories(5, 0, B)
    rng = np.random.default_rng(2)
    x0 = np.tile(np.array([0, 0, 3.0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0]), (B, 1))
    x0[:, :3] += rng.normal(0, 0.5, (B, 3)); x0[:, 7:10] += rng.normal(0, 1.0, (B, 3))
    outs = []
    for tune in (dict(groups=1, block_order=1), dict(groups=2, block_order=2)):
        e = Engine(_config(B, N, nb, 0, tune), lib_path=lib)
        assert e.get_groups() == (len(split) if tune["groups"] == 2 else 1)
        e.set_trajectories(traj, lens); e.sim_reset(x0)
        e.sim_steps(4, 2, 5e-3); e.sim_steps(2, 2, 5e-3)
        assert (e.get_status() == 0).all()
        order = e.get_block_order()
        if tune["block_order"] == 2:      # sorted inside each group: a permutation of the group's own indices
            b0 = 0
            for n in split:
                assert sorted(order[b0:b0 + n]) == list(range(b0, b0 + n)), order
                b0 += n
            assert b0 == B
        st = e.get_state()
        outs.append((*e.sim_get_state(), st["X"], st["U"], st["mu"], st["C"], st["idx"], e.get_tracking_stats()))
        e.close()
    assert (outs[0][6] == 6).all()
    for a, b in zip(*outs):
        assert np.array_equal(a, b)


ODD_BATCHES = [(13, (13,)), (21, (16, 5))]


# ------------------------------------------------------------------ emulator layer

@pytest.fixture(scope="module")
def emu():
    subprocess.check_call(["make", "-C", EMU_DIR], stdout=subprocess.DEVNULL)
    return EMU


@pytest.mark.parametrize("precision", [0, 1])
@pytest.mark.parametrize("N,nb", [s for s in SHAPES if s[0] <= 17])
def test_emu_shape_matrix(emu, N, nb, precision):
    _matrix_shape(emu, N, nb, precision)


def test_emu_shape_matrix_first_horizon_beyond_20(emu):
    _matrix_shape(emu, 21, 33, 0, layouts=(1,))


@pytest.mark.parametrize("precision", [0, 1])
@pytest.mark.parametrize("nb", BASIS_SIZES)
def test_emu_every_basis_point_in_play(emu, nb, precision):
    _every_basis_point(emu, nb, precision)


@pytest.mark.parametrize("precision", [0, 1])
def test_emu_largest_corner_is_refused(emu, precision):
    assert _corner(emu, 128, precision) is None


@pytest.mark.parametrize("precision", [0, 1])
@pytest.mark.parametrize("stage_mem", [1, 3], ids=["lds", "compact"])
@pytest.mark.parametrize("N,nb", SATURATED)
def test_emu_saturated_working_sets(emu, N, nb, stage_mem, precision):
    _saturated(emu, N, nb, precision, stage_mem, K=17)


@pytest.mark.parametrize("B,split", ODD_BATCHES, ids=["B13", "B21"])
def test_emu_groups_and_block_order_at_an_odd_batch(emu, B, split):
    _groups_odd_batch(emu, B, split)


# ------------------------------------------------------------------ GPU layer

@pytest.mark.gpu
@pytest.mark.parametrize("precision", [0, 1])
@pytest.mark.parametrize("N,nb", SHAPES)
def test_gpu_shape_matrix(N, nb, precision):
    _matrix_shape(None, N, nb, precision)


@pytest.mark.gpu
@pytest.mark.parametrize("precision", [0, 1])
@pytest.mark.parametrize("nb", BASIS_SIZES)
def test_gpu_every_basis_point_in_play(nb, precision):
    _every_basis_point(None, nb, precision)


@pytest.mark.gpu
@pytest.mark.parametrize("precision", [0, 1])
@pytest.mark.parametrize("nb", [128, 0])
def test_gpu_largest_corner(nb, precision):
    assert (_corner(None, nb, precision) is None) == (nb == 128)


@pytest.mark.gpu
@pytest.mark.parametrize("precision", [0, 1])
@pytest.mark.parametrize("stage_mem", [1, 2, 3], ids=["lds", "global", "compact"])
@pytest.mark.parametrize("N,nb", SATURATED)
def test_gpu_saturated_working_sets(N, nb, stage_mem, precision):
    _saturated(None, N, nb, precision, stage_mem, K=40)


@pytest.mark.gpu
@pytest.mark.parametrize("B,split", ODD_BATCHES, ids=["B13", "B21"])
def test_gpu_groups_and_block_order_at_an_odd_batch(B, split):
    _groups_odd_batch(None, B, split)

"""Loader of libmpcq.so (the HIP/gfx950 engine behind include/mpcq.h).

There is no CPU implementation of the engine in this package: if the shared library is missing
or no MI355X is visible, construction fails loudly (``MpcqError``)."""
from __future__ import annotations

import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_LIB = os.path.join(_HERE, "libmpcq.so")

_dp = ctypes.POINTER(ctypes.c_double)
_ip = ctypes.POINTER(ctypes.c_int32)
_lp = ctypes.POINTER(ctypes.c_int64)
_vp = ctypes.c_void_p


class NlOptions(ctypes.Structure):
    """mpcq_minsnap_nl_options (include/mpcq_nl_options.h): options of the min-snap generator's nonlinear stage."""
    _fields_ = [("time_penalty", ctypes.c_double), ("soft_constraint_weight", ctypes.c_double), ("soft_constraint_cap", ctypes.c_double),
                ("f_rel", ctypes.c_double), ("x_rel", ctypes.c_double), ("max_evaluations", ctypes.c_int32), ("time_cost", ctypes.c_int32),
                ("use_soft_constraints", ctypes.c_int32), ("reserved", ctypes.c_int32)]


def nl_defaults():
    """The defaults as the host library states them (mpcq_minsnap_nl_defaults = MPCQ_MINSNAP_NL_DEFAULTS), as a dict."""
    from .trajectories import _traj_lib
    d = _traj_lib().mpcq_minsnap_nl_defaults()
    return {name: getattr(d, name) for name, _ in NlOptions._fields_ if name != "reserved"}


def nl_options(opts=None):
    """NlOptions from a dict of overrides of the defaults (None: NULL, i.e. the library's defaults)."""
    if opts is None:
        return None
    base = nl_defaults()
    unknown = set(opts) - set(base)
    if unknown:
        raise ValueError(f"unknown nonlinear-stage options {sorted(unknown)}")
    return NlOptions(**{**base, **opts}, reserved=0)


_np = ctypes.POINTER(NlOptions)


class Leg(ctypes.Structure):
    """mpcq_leg (include/mpcq.h): kind, limits and radius of one leg of a device mission (mpcq_mission_set_legs)."""
    _fields_ = [("kind", ctypes.c_int32), ("reserved", ctypes.c_int32), ("v_max", ctypes.c_double), ("a_max", ctypes.c_double),
                ("radius", ctypes.c_double)]


_legp = ctypes.POINTER(Leg)


class TrainSpec(ctypes.Structure):
    """mpcq_train_spec (include/mpcq.h): what mpcq_rgp_train / mpcq_record_train train and with which model."""
    _fields_ = [("mode", ctypes.c_int32), ("pair_next", ctypes.c_int32), ("nb", ctypes.c_int32), ("basis", _dp), ("theta", _dp)]


class TrainOut(ctypes.Structure):
    """mpcq_train_out (include/mpcq.h): host arrays of the trained state, each may be NULL."""
    _fields_ = [("mu", _dp), ("C", _dp), ("mu_eta", _dp), ("C_eta", _dp), ("Kx_inv", _dp)]


TRAIN_MODES = {"regress": 1, "learn": 2}
_tsp = ctypes.POINTER(TrainSpec)
_top = ctypes.POINTER(TrainOut)

# every symbol declared in include/mpcq.h: (name, restype, argtypes)
SYMBOLS = [
    ("mpcq_last_error", ctypes.c_char_p, []),
    ("mpcq_version", ctypes.c_char_p, []),
    ("mpcq_create", ctypes.c_int, [_vp, ctypes.POINTER(_vp)]),
    ("mpcq_create_sized", ctypes.c_int, [_vp, ctypes.c_uint64, ctypes.POINTER(_vp)]),
    ("mpcq_destroy", ctypes.c_int, [_vp]),
    ("mpcq_reset", ctypes.c_int, [_vp]),
    ("mpcq_set_trajectories", ctypes.c_int, [_vp, _dp, _ip, ctypes.c_int32]),
    ("mpcq_set_reference", ctypes.c_int, [_vp, _dp, _dp]),
    ("mpcq_set_params", ctypes.c_int, [_vp, _dp]),
    ("mpcq_solve", ctypes.c_int, [_vp, _dp]),
    ("mpcq_get_x", ctypes.c_int, [_vp, ctypes.c_int32, _dp]),
    ("mpcq_get_u", ctypes.c_int, [_vp, ctypes.c_int32, _dp]),
    ("mpcq_get_cost", ctypes.c_int, [_vp, _dp]),
    ("mpcq_get_status", ctypes.c_int, [_vp, _ip]),
    ("mpcq_get_qp_iter", ctypes.c_int, [_vp, _ip]),
    ("mpcq_get_qp_work", ctypes.c_int, [_vp, _ip]),
    ("mpcq_get_stats", ctypes.c_int, [_vp, _dp]),
    ("mpcq_predict_nominal", ctypes.c_int, [_vp, _dp, _dp, ctypes.c_double, _dp]),
    ("mpcq_rgp_regress", ctypes.c_int, [_vp, _dp, _dp]),
    ("mpcq_get_rgp", ctypes.c_int, [_vp, _dp, _dp]),
    ("mpcq_step", ctypes.c_int, [_vp, _dp, _dp, _dp]),
    ("mpcq_step_device_async", ctypes.c_int, [_vp, _vp, _vp]),
    ("mpcq_synchronize", ctypes.c_int, [_vp]),
    ("mpcq_stream", _vp, [_vp]),
    ("mpcq_get_command", ctypes.c_int, [_vp, _dp, _dp, _dp]),
    ("mpcq_get_finished", ctypes.c_int, [_vp, _ip]),
    ("mpcq_get_reference_chunk", ctypes.c_int, [_vp, _dp]),
    ("mpcq_plant_substeps", ctypes.c_int, [ctypes.c_double, ctypes.c_double]),
    ("mpcq_sim_plant_period", ctypes.c_int, [_vp, _dp, ctypes.c_double, ctypes.c_double, _ip]),
    ("mpcq_sim_control_periods", ctypes.c_int, [_vp, ctypes.c_int32, ctypes.c_double, ctypes.c_double, _ip]),
    ("mpcq_sim_reset", ctypes.c_int, [_vp, _dp]),
    ("mpcq_sim_steps", ctypes.c_int, [_vp, ctypes.c_int32, ctypes.c_int32, ctypes.c_double]),
    ("mpcq_sim_run", ctypes.c_int, [_vp, ctypes.c_int32, ctypes.c_int32, ctypes.c_double]),
    ("mpcq_sim_get_state", ctypes.c_int, [_vp, _dp, _dp]),
    ("mpcq_get_kernel_time", ctypes.c_int, [_vp, _dp, _ip]),
    ("mpcq_get_kernel_time_minmax", ctypes.c_int, [_vp, _dp, _dp]),
    ("mpcq_debug_profile", ctypes.c_int, [_vp, _vp]),
    ("mpcq_get_block_order", ctypes.c_int, [_vp, _ip]),
    ("mpcq_get_groups", ctypes.c_int, [_vp, _ip]),
    ("mpcq_get_tracking_stats", ctypes.c_int, [_vp, _dp]),
    ("mpcq_comm_unique_id", ctypes.c_int, [_vp]),
    ("mpcq_comm_init", ctypes.c_int, [_vp, ctypes.c_int32, ctypes.c_int32, _vp]),
    ("mpcq_comm_share", ctypes.c_int, [_vp, _vp]),
    ("mpcq_allreduce_tracking_stats", ctypes.c_int, [_vp, _dp]),
    ("mpcq_get_state", ctypes.c_int, [_vp, _dp, _dp, _dp, _dp, _dp, _ip, _ip]),
    ("mpcq_set_state", ctypes.c_int, [_vp, _dp, _dp, _dp, _dp, _dp, _ip, _ip]),
    ("mpcq_get_solver_state", ctypes.c_int, [_vp, _ip, _dp, _ip]),
    ("mpcq_set_solver_state", ctypes.c_int, [_vp, _ip, _dp, _ip]),
    ("mpcq_replan", ctypes.c_int, [_vp, _dp, _dp, ctypes.c_int32, ctypes.c_double, ctypes.c_double, ctypes.c_int32, ctypes.c_double, _ip, _ip]),
    ("mpcq_replan_nonlinear", ctypes.c_int, [_vp, _dp, _dp, ctypes.c_int32, ctypes.c_double, ctypes.c_double, ctypes.c_int32, ctypes.c_double, _ip,
                                             _ip, _np, _dp, _dp, _dp]),
    ("mpcq_replan_circle", ctypes.c_int, [_vp, _dp, _dp, _dp, ctypes.c_int32, ctypes.c_double, ctypes.c_double, _ip, _ip]),
    ("mpcq_replace_trajectories", ctypes.c_int, [_vp, _ip, ctypes.c_int32, _dp, _ip]),
    ("mpcq_get_trajectories", ctypes.c_int, [_vp, _dp, _ip]),
    ("mpcq_mission_set", ctypes.c_int, [_vp, _dp, ctypes.c_int32, ctypes.c_int32, ctypes.c_double, ctypes.c_double, ctypes.c_int32, ctypes.c_double,
                                        ctypes.c_int32, _np, _ip]),
    ("mpcq_mission_set_legs", ctypes.c_int, [_vp, _legp, _dp, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_double, ctypes.c_int32, _np,
                                             _ip]),
    ("mpcq_mission_get", ctypes.c_int, [_vp, _ip, _ip, _ip, _ip, _ip, _dp]),
    ("mpcq_mission_stop", ctypes.c_int, [_vp]),
    ("mpcq_record_start", ctypes.c_int, [_vp, _ip, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32]),
    ("mpcq_record_info", ctypes.c_int, [_vp, _ip, _lp, _lp]),
    ("mpcq_record_get", ctypes.c_int, [_vp, ctypes.c_int32, _dp]),
    ("mpcq_record_get_solver", ctypes.c_int, [_vp, _ip]),
    ("mpcq_record_get_periods", ctypes.c_int, [_vp, _lp]),
    ("mpcq_record_clear", ctypes.c_int, [_vp]),
    ("mpcq_record_stop", ctypes.c_int, [_vp]),
    ("mpcq_score_start", ctypes.c_int, [_vp, ctypes.c_int32, ctypes.c_int32]),
    ("mpcq_score_get", ctypes.c_int, [_vp, _dp, _ip, _ip, _lp]),
    ("mpcq_score_clear", ctypes.c_int, [_vp]),
    ("mpcq_score_stop", ctypes.c_int, [_vp]),
    ("mpcq_rgp_predict", ctypes.c_int, [_vp, _dp, ctypes.c_int32, ctypes.c_int32, _dp, _dp]),
    ("mpcq_record_predict", ctypes.c_int, [_vp, _dp, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _dp, _dp]),
    ("mpcq_rgp_train", ctypes.c_int, [_vp, _tsp, _dp, _dp, ctypes.c_int32, ctypes.c_int32, _top]),
    ("mpcq_record_train", ctypes.c_int, [_vp, _tsp, ctypes.c_int32, ctypes.c_int32, _top]),
    ("mpcq_fleet_set", ctypes.c_int, [_vp, _vp, ctypes.c_uint64, ctypes.c_int64]),
    ("mpcq_fleet_get", ctypes.c_int, [_vp, _vp, ctypes.c_uint64, _lp]),
    ("mpcq_fleet_stop", ctypes.c_int, [_vp]),
    ("mpcq_sensor_start", ctypes.c_int, [_vp, _vp, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32]),
    ("mpcq_sensor_get", ctypes.c_int, [_vp, _dp, _ip, _lp]),
    ("mpcq_sensor_sample", ctypes.c_int, [_vp, _dp]),
    ("mpcq_sensor_stop", ctypes.c_int, [_vp]),
    ("mpcq_explore_start", ctypes.c_int, [_vp, _vp, ctypes.c_uint64, _vp, _dp, _lp]),
    ("mpcq_explore_get", ctypes.c_int, [_vp, _dp, _lp, _dp]),
    ("mpcq_explore_stop", ctypes.c_int, [_vp]),
    ("mpcq_blackbox_start", ctypes.c_int, [_vp, _ip, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _vp]),
    ("mpcq_blackbox_info", ctypes.c_int, [_vp, _lp, _ip, _ip, _ip, _ip, _lp]),
    ("mpcq_blackbox_get", ctypes.c_int, [_vp, ctypes.c_int32, _ip, ctypes.c_int32, _dp]),
    ("mpcq_blackbox_get_solver", ctypes.c_int, [_vp, _ip, ctypes.c_int32, _ip]),
    ("mpcq_blackbox_get_periods", ctypes.c_int, [_vp, _ip, ctypes.c_int32, _lp]),
    ("mpcq_blackbox_rearm", ctypes.c_int, [_vp, _ip]),
    ("mpcq_blackbox_stop", ctypes.c_int, [_vp]),
    ("mpcq_learn_last_error", ctypes.c_char_p, []),
    ("mpcq_learn_create", ctypes.c_int, [ctypes.c_int32, ctypes.c_int32, _dp, _dp, ctypes.c_int32, ctypes.POINTER(_vp)]),
    ("mpcq_learn_destroy", ctypes.c_int, [_vp]),
    ("mpcq_learn_step", ctypes.c_int, [_vp, _dp, _dp]),
    ("mpcq_learn_get", ctypes.c_int, [_vp, _dp, _dp, _dp, _dp, _dp]),
]


class MpcqError(RuntimeError):
    pass


_cache = {}


def load(path: str | None = None):
    path = os.path.abspath(path or os.environ.get("MPCQ_LIB") or DEFAULT_LIB)   # MPCQ_LIB: experiment builds (csrc/Makefile `variant`)
    if path in _cache:
        return _cache[path]
    if not os.path.exists(path):
        raise MpcqError(
            f"{path} not found: build it with `make -C mpc_quad_ros_amd/csrc` (hipcc, gfx950). "
            "This package has no CPU implementation of the control step.")
    lib = ctypes.CDLL(path)
    for name, res, args in SYMBOLS:
        fn = getattr(lib, name)      # AttributeError if the ABI is incomplete
        fn.restype = res
        fn.argtypes = args
    _cache[path] = lib
    return lib


def d(a):
    return None if a is None else a.ctypes.data_as(_dp)


def i(a):
    return None if a is None else a.ctypes.data_as(_ip)


def l(a):
    return None if a is None else a.ctypes.data_as(_lp)

"""Quadrotor constants, OCP weights and engine configuration.

Plain data shared by the host facade, the tests and the bench.  Values and their
provenance in the reference (paths relative to the reference checkout):

* hummingbird(): ``Quadrotor3D.set_parameters_from_file`` src/quad.py:385-417 applied to
  config/hummingbird.xacro:29-50 ('+' layout, flipped z_l_tau sign, src/quad.py:414-417).
* legacy_sim(): the constants the shipped python-simulation logs were produced with
  (mass 1.0, max_thrust 20, J=[.03,.03,.06], arm .235, c .013) — the *current*
  defaults at src/quad.py:41-67 (mass 0.03, arm 0.04) match no log.
* weights: src/quad_opt.py:122-130; input bounds src/quad_opt.py:142-144; hover reference
  u_ref = 0.16 src/quad_opt.py:304.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass, field
from typing import Optional, Sequence

import numpy as np

NX, NU, NY = 13, 4, 17


@dataclass
class QuadParams:
    mass: float
    J: Sequence[float]
    max_thrust: float
    x_f: Sequence[float]
    y_f: Sequence[float]
    z_l_tau: Sequence[float]
    g: float = 9.81                      # src/quad.py:73
    rotor_drag: Sequence[float] = (0.3, 0.3, 0.0)   # src/quad.py:79-84 (plant only)
    aero_drag: float = 0.008             # src/quad.py:89 (plant only)


def hummingbird() -> QuadParams:
    L, c = 0.17, 0.016
    return QuadParams(
        mass=0.68 + 4 * 0.009,
        J=(0.007, 0.007, 0.012),
        max_thrust=838.0 ** 2 * 8.54858e-06,
        x_f=(L, 0.0, -L, 0.0),
        y_f=(0.0, L, 0.0, -L),
        z_l_tau=(c, -c, c, -c),          # -[-c, c, -c, c], src/quad.py:417
    )


def legacy_sim() -> QuadParams:
    L, c = 0.47 / 2, 0.013
    return QuadParams(
        mass=1.0,
        J=(0.03, 0.03, 0.06),
        max_thrust=20.0,
        x_f=(L, 0.0, -L, 0.0),
        y_f=(0.0, L, 0.0, -L),
        z_l_tau=(-c, c, -c, c),
    )


def default_W() -> np.ndarray:
    # q_cost with the mean attitude weight inserted for the 4th quaternion component, then r_cost
    q_cost = np.array([10, 10, 10, 0.1, 0.1, 0.1, 0.05, 0.05, 0.05, 0.05, 0.05, 0.05])
    q_diag = np.concatenate((q_cost[:3], np.mean(q_cost[3:6])[np.newaxis], q_cost[3:]))
    return np.concatenate((q_diag, np.full(4, 0.1)))


class CTuning(ctypes.Structure):
    """Binary layout of ``mpcq_tuning`` (include/mpcq.h); every field 0 = default."""
    _fields_ = [
        ("warm_max", ctypes.c_int32), ("warm_retry", ctypes.c_int32), ("flip_max", ctypes.c_int32),
        ("abort_pins", ctypes.c_int32), ("abort_wrong", ctypes.c_int32), ("polish_max", ctypes.c_int32),
        ("stage_mem", ctypes.c_int32), ("generic_kernel", ctypes.c_int32),
        ("pin_ratio", ctypes.c_double), ("ipm_mu0", ctypes.c_double), ("ipm_margin", ctypes.c_double), ("ipm_tol", ctypes.c_double),
        ("block_order", ctypes.c_int32),     # since 0.4
        ("groups", ctypes.c_int32),          # since 0.6 (0.4 / 0.5: reserved, 0)
    ]


STAGE_MEM = {"auto": 0, "lds": 1, "global": 2, "compact": 3}


class CConfig(ctypes.Structure):
    """Binary layout of ``mpcq_config`` (include/mpcq.h); the oracle's ``orc_config`` has the
    same leading fields (it ignores device / precision / qp options)."""
    _fields_ = [
        ("batch", ctypes.c_int32), ("N", ctypes.c_int32), ("nb", ctypes.c_int32), ("skip", ctypes.c_int32),
        ("T", ctypes.c_double), ("dt_pred", ctypes.c_double),
        ("mass", ctypes.c_double), ("J", ctypes.c_double * 3), ("max_thrust", ctypes.c_double),
        ("x_f", ctypes.c_double * 4), ("y_f", ctypes.c_double * 4), ("z_l_tau", ctypes.c_double * 4),
        ("g", ctypes.c_double),
        ("rotor_drag", ctypes.c_double * 3), ("aero_drag", ctypes.c_double),
        ("W", ctypes.c_double * 17), ("W_e", ctypes.c_double * 13),
        ("u_lb", ctypes.c_double * 4), ("u_ub", ctypes.c_double * 4), ("u_ref", ctypes.c_double * 4),
        ("qp_tol", ctypes.c_double),
        ("basis", ctypes.POINTER(ctypes.c_double)), ("theta", ctypes.POINTER(ctypes.c_double)),
        # --- product-only tail (the oracle's struct ends above)
        ("device", ctypes.c_int32), ("precision", ctypes.c_int32),
        ("qp_max_iter", ctypes.c_int32), ("flags", ctypes.c_int32),
        ("finish_radius", ctypes.c_double),
        ("tune", CTuning),
    ]


PRECISION_F64 = 0
PRECISION_F32 = 1


@dataclass
class EngineConfig:
    """One engine = B independent quadrotors sharing (N, T, nb, quad constants, theta)."""
    batch: int
    N: int = 20                       # n_nodes
    T: float = 1.0                    # t_lookahead
    quad: QuadParams = field(default_factory=hummingbird)
    nb: int = 0                       # basis points per axis (0: no GP in the model)
    basis: Optional[np.ndarray] = None    # [3, nb]
    theta: Optional[np.ndarray] = None    # [3, 3] rows = (L, sigma_f, sigma_n) per axis
    dt_pred: float = 0.01             # ODOMETRY_DT (node) / optimization_dt (python sim)
    skip: Optional[int] = None        # control_freq_factor; default int((T/N)/0.01) as the node
    W: np.ndarray = field(default_factory=default_W)
    W_e: Optional[np.ndarray] = None
    u_lb: Sequence[float] = (0.0, 0.0, 0.0, 0.0)
    u_ub: Sequence[float] = (1.0, 1.0, 1.0, 1.0)
    u_ref: Sequence[float] = (0.16, 0.16, 0.16, 0.16)
    qp_tol: float = 0.0               # 0 -> implementation default
    device: int = 0
    precision: int = PRECISION_F64
    qp_max_iter: int = 0              # 0 -> implementation default
    static_gp: bool = False           # MPCQ_FLAG_STATIC_GP: fixed GP in the model (use_gp = 1), no recursive update in the step
    finish_radius: float = 0.0        # EPSILON_TRAJECTORY_FINISHED [m]; 0 -> 1.0 (src/mpc_controller_node.py:118)
    tune: Optional[dict] = None       # mpcq_tuning fields by name (include/mpcq.h); stage_mem also as "lds" / "global"

    def __post_init__(self):
        if self.skip is None:
            # src/mpc_controller_node.py:222
            self.skip = int((self.T / self.N) / 0.01)
        if self.W_e is None:
            self.W_e = np.asarray(self.W)[:NX].copy()
        if self.nb:
            if self.basis is None:
                raise ValueError("nb > 0 needs basis[3, nb]")
            self.basis = np.ascontiguousarray(np.asarray(self.basis, dtype=np.float64).reshape(3, self.nb))
            if self.theta is None:
                self.theta = np.tile(np.array([1.0, 0.1, 0.1]), (3, 1))   # RGP default, src/gp/RGP.py:106
            th = np.asarray(self.theta, dtype=np.float64)
            if th.shape == (3,):
                th = np.tile(th, (3, 1))
            self.theta = np.ascontiguousarray(th.reshape(3, 3))
        else:
            self.basis = np.zeros((3, 0))
            self.theta = np.zeros((3, 3))

    @property
    def optimization_dt(self) -> float:
        return self.T / self.N

    def to_c(self) -> CConfig:
        c = CConfig()
        c.batch, c.N, c.nb, c.skip = self.batch, self.N, self.nb, int(self.skip)
        c.T, c.dt_pred = float(self.T), float(self.dt_pred)
        q = self.quad
        c.mass, c.max_thrust, c.g, c.aero_drag = q.mass, q.max_thrust, q.g, q.aero_drag
        c.J[:] = list(q.J); c.x_f[:] = list(q.x_f); c.y_f[:] = list(q.y_f); c.z_l_tau[:] = list(q.z_l_tau)
        c.rotor_drag[:] = list(q.rotor_drag)
        c.W[:] = [float(v) for v in self.W]; c.W_e[:] = [float(v) for v in self.W_e]
        c.u_lb[:] = list(self.u_lb); c.u_ub[:] = list(self.u_ub); c.u_ref[:] = list(self.u_ref)
        c.qp_tol = float(self.qp_tol)
        self._basis_buf = np.ascontiguousarray(self.basis.ravel(), dtype=np.float64)
        self._theta_buf = np.ascontiguousarray(self.theta.ravel(), dtype=np.float64)
        c.basis = self._basis_buf.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
        c.theta = self._theta_buf.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
        c.device, c.precision, c.qp_max_iter, c.flags = self.device, self.precision, self.qp_max_iter, (1 if self.static_gp else 0)
        c.finish_radius = float(self.finish_radius)
        for k, v in (self.tune or {}).items():
            if k not in dict(CTuning._fields_):
                raise ValueError(f"unknown tuning field {k!r}")
            if k == "stage_mem" and isinstance(v, str):
                v = STAGE_MEM[v]
            setattr(c.tune, k, v)
        return c


def static_gp_theta(theta):
    """Hyper-parameters of a static GP (src/gp/GP.py:113-130: K + (noise + 1e-7) I with noise = theta[-1], NOT squared) in
    the engine's convention K_x = K + sigma_n^2 I: [L, sigma_f, sqrt(noise + 1e-7)]."""
    th = np.asarray(theta, dtype=np.float64)
    if th.ndim == 1:
        return np.array([th[0], th[-2], np.sqrt(th[-1] + 1e-7)])
    return np.stack([static_gp_theta(t) for t in th])


def rgp_basis_linspace(v_max: float, nb: int) -> np.ndarray:
    """Node basis: np.linspace(-v_max, v_max, nb) on each axis, src/mpc_controller_node.py:212."""
    return np.tile(np.linspace(-v_max, v_max, nb), (3, 1))


# ---------------------------------------------------------------------------------------------
# The fleet (include/mpcq.h mpcq_fleet_*): every quadrotor its own plant -- the reference's whole Quadrotor3D (src/quad.py:36-94), with
# payload, rotor functionality and body-frame disturbances, while the controller keeps the engine's model.
PLANT_DTYPE = np.dtype([
    ("mass", np.float64), ("J", np.float64, (3,)), ("max_thrust", np.float64),
    ("x_f", np.float64, (4,)), ("y_f", np.float64, (4,)), ("z_l_tau", np.float64, (4,)),
    ("rotor_drag", np.float64, (3,)), ("aero_drag", np.float64), ("payload_mass", np.float64),
    ("rotor_functionality", np.float64, (4,)), ("f_d", np.float64, (3,)), ("t_d", np.float64, (3,)),
    ("d_from", np.int32), ("d_to", np.int32)], align=True)
"""Binary layout of ``mpcq_plant`` (include/mpcq.h)."""


def fleet_defaults(cfg: "EngineConfig | QuadParams", count: int) -> np.ndarray:
    """`count` plants that restate the engine's own (cfg: an EngineConfig or its QuadParams): payload 0, every rotor functional, no
    disturbance.  Flying them is bit for bit flying without a fleet; the start of every hand-made table."""
    q = cfg.quad if isinstance(cfg, EngineConfig) else cfg
    p = np.zeros(count, PLANT_DTYPE)
    p["mass"], p["max_thrust"], p["aero_drag"] = q.mass, q.max_thrust, q.aero_drag
    for name in ("J", "x_f", "y_f", "z_l_tau", "rotor_drag"):
        p[name] = np.asarray(getattr(q, name), dtype=np.float64)
    p["rotor_functionality"] = 1.0
    return p


def fleet_sample(seed: int, first_index: int, count: int, cfg: "EngineConfig | QuadParams", spread: float = 1.3, payload_max: float = 0.0,
                 fault_prob: float = 0.0, fault_min: float = 0.5, gust_force: float = 0.0, gust_torque: float = 0.0, gust_window=(0, 0)) -> np.ndarray:
    """A randomised fleet around the engine's plant, quadrotors first_index .. first_index + count - 1 of it.  Every quadrotor is drawn
    from a generator of its own, seeded with (seed, global index), so shards of a swarm agree with the whole (as swarm_trajectories).
      spread       mass, each J, max_thrust, each rotor drag and the aero drag are multiplied by independent factors, log-uniform in
                   [1 / spread, spread] (1: unchanged); a float, or a dict by field name ('mass', 'J', 'max_thrust', 'rotor_drag', 'aero_drag')
      payload_max  payload_mass uniform in [0, payload_max] kg
      fault_prob   with this probability ONE rotor of the quadrotor, picked uniformly, has functionality uniform in [fault_min, 1]
      gust_force, gust_torque   standard deviations [N], [N m] of the normal body-frame f_d, t_d, which act in the fleet periods
                   gust_window = (d_from, d_to)"""
    p = fleet_defaults(cfg, count)
    sp = spread if isinstance(spread, dict) else {k: spread for k in ("mass", "J", "max_thrust", "rotor_drag", "aero_drag")}
    unknown = set(sp) - {"mass", "J", "max_thrust", "rotor_drag", "aero_drag"}
    if unknown or any(not v >= 1.0 for v in sp.values()):
        raise ValueError("spread: factors >= 1 for mass, J, max_thrust, rotor_drag, aero_drag")
    if not 0.0 <= fault_prob <= 1.0 or not 0.0 <= fault_min <= 1.0 or payload_max < 0:
        raise ValueError("fault_prob and fault_min in [0, 1], payload_max >= 0")
    for i in range(count):
        rng = np.random.default_rng([int(seed), int(first_index) + i])
        # (every draw is made whatever the options, so that one option does not move the others' values)
        f = {k: np.exp(rng.uniform(-1.0, 1.0, n)) for k, n in (("mass", 1), ("J", 3), ("max_thrust", 1), ("rotor_drag", 3), ("aero_drag", 1))}
        pay, hit, rotor, level = rng.uniform(), rng.uniform(), rng.integers(4), rng.uniform()
        fd, td = rng.normal(size=3), rng.normal(size=3)
        for k, v in f.items():
            fac = v ** np.log(sp.get(k, 1.0))
            p[k][i] = p[k][i] * (fac if fac.size > 1 else fac[0])
        p["payload_mass"][i] = pay * payload_max
        if hit < fault_prob:
            p["rotor_functionality"][i, rotor] = fault_min + (1.0 - fault_min) * level
        p["f_d"][i], p["t_d"][i] = gust_force * fd + 0.0, gust_torque * td + 0.0   # (+ 0.0: no -0.0 where there is no gust)
    p["d_from"], p["d_to"] = int(gust_window[0]), int(gust_window[1])
    return p


def fleet_drag_accel(plants: np.ndarray, v) -> np.ndarray:
    """Body-frame drag acceleration of every plant at body velocities v, Quadrotor3D.get_aero_drag(body_frame=True) (src/quad.py:256-277):
    -aero_drag v^2 sign(v) / mass - rotor_drag v / mass.  v [M] (one grid for all axes), [3, M] or [B, 3, M] -> [B, 3, M]."""
    plants = np.asarray(plants)
    v = np.asarray(v, dtype=np.float64)
    B = plants.shape[0]
    if v.ndim == 1:
        v = np.tile(v, (3, 1))
    v = np.broadcast_to(v, (B,) + v.shape[-2:])
    mass = plants["mass"][:, None, None]
    a = -plants["aero_drag"][:, None, None] * v ** 2 * np.sign(v) / mass
    a -= plants["rotor_drag"][:, :, None] * v / mass
    return a


# ---------------------------------------------------------------------------------------------
# The sensor (include/mpcq.h mpcq_sensor_*): white noise, bias, latency, dropout and an outage window per quadrotor, between the plant
# and the controller of sim_steps.
SENSOR_JUDGE_MEASURED, SENSOR_JUDGE_TRUTH = 0, 1
SENSOR_DTYPE = np.dtype([
    ("sigma_p", np.float64, (3,)), ("sigma_att", np.float64, (3,)), ("sigma_v", np.float64, (3,)), ("sigma_r", np.float64, (3,)),
    ("bias_p", np.float64, (3,)), ("bias_att", np.float64, (3,)), ("bias_v", np.float64, (3,)), ("bias_r", np.float64, (3,)),
    ("p_drop", np.float64), ("delay", np.int32), ("reserved", np.int32), ("out_from", np.int64), ("out_to", np.int64)], align=True)
"""Binary layout of ``mpcq_sensor`` (include/mpcq.h)."""
SENSOR_CHANNELS = ("p", "att", "v", "r")


def sensor_defaults(count: int) -> np.ndarray:
    """`count` sensors that measure the identity (all zero): flying them is bit for bit flying without a sensor."""
    return np.zeros(count, SENSOR_DTYPE)


def sensor_sample(seed: int, first_index: int, count: int, sigma=None, bias=None, p_drop_max: float = 0.0, delay_max: int = 0,
                  outage_prob: float = 0.0, outage=(0, 0)) -> np.ndarray:
    """Randomised sensors, quadrotors first_index .. first_index + count - 1 of a swarm.  Every quadrotor is drawn from a generator of
    its own, seeded with (seed, global index), so shards of a swarm agree with the whole (as fleet_sample).
      sigma        dict by channel ('p', 'att', 'v', 'r'): each of the three standard deviations uniform in [0, value]
      bias         dict by channel: each of the three offsets normal with this standard deviation
      p_drop_max   p_drop uniform in [0, p_drop_max]
      delay_max    delay uniform in {0, .., delay_max} (sensor_start needs depth > delay_max)
      outage_prob  with this probability the quadrotor has the outage window outage = (out_from, out_to)"""
    s = sensor_defaults(count)
    sigma, bias = dict(sigma or {}), dict(bias or {})
    unknown = (set(sigma) | set(bias)) - set(SENSOR_CHANNELS)
    if unknown or any(not v >= 0 for v in list(sigma.values()) + list(bias.values())):
        raise ValueError("sigma and bias: values >= 0 by channel 'p', 'att', 'v', 'r'")
    if not 0.0 <= p_drop_max <= 1.0 or not 0.0 <= outage_prob <= 1.0 or delay_max < 0:
        raise ValueError("p_drop_max and outage_prob in [0, 1], delay_max >= 0")
    for i in range(count):
        rng = np.random.default_rng([int(seed), int(first_index) + i])
        # (every draw is made whatever the options, so that one option does not move the others' values)
        us, ns = rng.uniform(size=(4, 3)), rng.normal(size=(4, 3))
        drop, delay, hit = rng.uniform(), rng.uniform(), rng.uniform()
        for k, ch in enumerate(SENSOR_CHANNELS):
            s["sigma_" + ch][i] = sigma.get(ch, 0.0) * us[k]
            s["bias_" + ch][i] = bias.get(ch, 0.0) * ns[k] + 0.0   # (+ 0.0: no -0.0 where there is no bias)
        s["p_drop"][i] = p_drop_max * drop
        s["delay"][i] = min(int(delay * (delay_max + 1)), delay_max)
        if hit < outage_prob:
            s["out_from"][i], s["out_to"][i] = int(outage[0]), int(outage[1])
    return s


# ---------------------------------------------------------------------------------------------
# Exploration (include/mpcq.h mpcq_explore_*): the limits of the next mission leg from the envelope of body velocities a quadrotor has
# flown -- the reference's Explorer (src/Explorer.py:40-84) as src/explore_trajectories.py:59-125 applies it, per quadrotor on the device.
EXPLORE_LAST_FLIGHT, EXPLORE_CUMULATIVE = 0, 1
EXPLORE_RULE_DTYPE = np.dtype([("step", np.float64), ("desired", np.float64), ("v_limit", np.float64), ("a_limit", np.float64),
                               ("mode", np.int32), ("axes", np.int32)], align=True)
"""Binary layout of ``mpcq_explore_rule`` (include/mpcq.h)."""


def explore_rules(B: int, step=10.0, desired=20.0, v_limit=30.0, a_limit=30.0, mode=EXPLORE_LAST_FLIGHT, axes=7) -> np.ndarray:
    """B rules for Engine.explore_start; every argument a scalar or [B].  The defaults are the reference's numbers: exploration_step 10,
    desired_explored_vmax 20 (src/Explorer.py:26-27), v_max_limit = a_max_limit = 30 (src/explore_trajectories.py:67-68), a fresh GP per
    run (mode 0) and all three axes (axes 7; bit i: axis i)."""
    r = np.zeros(B, EXPLORE_RULE_DTYPE)
    r["step"], r["desired"], r["v_limit"], r["a_limit"], r["mode"], r["axes"] = step, desired, v_limit, a_limit, mode, axes
    return r


def explore_velocity(env, samples, rules):
    """The rule on the host, vectorised over B: (explored, v_max, a_max), each [B], from env [B, 3, 2] (min, max of v_body per axis),
    samples [B] (0: the envelope reads as all zero) and rules [B] of EXPLORE_RULE_DTYPE.  Per axis vabs = 0, raised to max if max > vabs,
    then to |min| if |min| > vabs; explored = the smallest vabs over the axes of `axes`; v = explored + step if that is < desired, else
    desired; v_max = v_limit if v > v_limit else v, a_max likewise with a_limit."""
    env = np.where(np.asarray(samples).reshape(-1, 1, 1) > 0, np.asarray(env, dtype=np.float64), 0.0)
    mn, mx = env[:, :, 0], env[:, :, 1]
    vabs = np.zeros(mx.shape)
    vabs = np.where(mx > vabs, mx, vabs)
    vabs = np.where(np.abs(mn) > vabs, np.abs(mn), vabs)
    use = (np.asarray(rules["axes"])[:, None] >> np.arange(3)) & 1 != 0
    explored = np.where(use, vabs, np.inf).min(axis=1)
    nxt = explored + rules["step"]
    v = np.where(nxt < rules["desired"], nxt, rules["desired"])
    return explored, np.where(v > rules["v_limit"], rules["v_limit"], v), np.where(v > rules["a_limit"], rules["a_limit"], v)


# ---------------------------------------------------------------------------------------------
# Incident recorder (include/mpcq.h mpcq_blackbox_*): a ring of the flight recorder's rows per watched quadrotor, stopped by a rule of its
# own that the device judges every period.
BB_STATUS, BB_FALLBACK, BB_NONFINITE, BB_ERR_POS, BB_SPEED, BB_TILT, BB_COST = 1, 2, 4, 8, 16, 32, 64
BB_CAUSES = {"status": BB_STATUS, "fallback": BB_FALLBACK, "nonfinite": BB_NONFINITE, "err_pos": BB_ERR_POS, "speed": BB_SPEED,
             "tilt": BB_TILT, "cost": BB_COST}
BLACKBOX_RULE_DTYPE = np.dtype([("causes", np.int32), ("status_mask", np.int32), ("err_pos", np.float64), ("speed", np.float64),
                                ("tilt_cos", np.float64), ("cost", np.float64)], align=True)
"""Binary layout of ``mpcq_blackbox_rule`` (include/mpcq.h)."""


def blackbox_rules(count: int, status_mask=0, fallback=False, nonfinite=True, err_pos=None, speed=None, tilt_cos=None, cost=None) -> np.ndarray:
    """`count` rules for Engine.blackbox_start; every argument a scalar or [count].  status_mask: the status bits that raise BB_STATUS
    (0: off); fallback, nonfinite: whether a fallback solve / a non-finite measurement, control or cost fires; err_pos [m], speed [m/s],
    tilt_cos (cosine of the angle between body z and world z) and cost: thresholds, None or NaN (per entry) for a cause that is off."""
    r = np.zeros(count, BLACKBOX_RULE_DTYPE)
    r["status_mask"] = status_mask
    r["causes"] = np.where(r["status_mask"] != 0, BB_STATUS, 0)
    r["causes"] |= np.where(np.broadcast_to(np.asarray(fallback, dtype=bool), (count,)), BB_FALLBACK, 0).astype(np.int32)
    r["causes"] |= np.where(np.broadcast_to(np.asarray(nonfinite, dtype=bool), (count,)), BB_NONFINITE, 0).astype(np.int32)
    for name, bit, v in (("err_pos", BB_ERR_POS, err_pos), ("speed", BB_SPEED, speed), ("tilt_cos", BB_TILT, tilt_cos), ("cost", BB_COST, cost)):
        if v is None:
            continue
        v = np.broadcast_to(np.asarray(v, dtype=np.float64), (count,))
        on = ~np.isnan(v)
        r[name] = np.where(on, v, 0.0)
        r["causes"] |= np.where(on, bit, 0).astype(np.int32)
    return r


def blackbox_causes(rows, rules) -> np.ndarray:
    """The device's judge on the host: the cause word [count, T] (int32) of every row of a record_get()-shaped dict `rows` (x_odom, x_ref,
    w_odom, cost_solution, status, qp_iter -- a key is needed only if a cause that reads it is enabled) under rules [count] of
    BLACKBOX_RULE_DTYPE, with the device's expressions in the device's order: numpy rounds every operation on its own, as the kernel
    does.  The first period at which a quadrotor's word is non-zero is where its black box fires, with that word as the cause; tune
    thresholds on a recording with it."""
    rules = np.asarray(rules)
    en = rules["causes"].astype(np.int32)[:, None]
    shape = None
    for k in ("x_odom", "cost_solution", "status", "qp_iter", "w_odom", "x_ref"):
        if k in rows:
            shape = np.asarray(rows[k]).shape[:2]
            break
    if shape is None:
        raise ValueError("rows holds none of the fields the rule reads")
    if shape[0] != len(rules):
        raise ValueError(f"rows is for {shape[0]} quadrotors, rules for {len(rules)}")
    c = np.zeros(shape, np.int32)

    def need(bit, *keys):
        if not (en & bit).any():
            return False
        missing = [k for k in keys if k not in rows]
        if missing:
            raise ValueError(f"cause {bit} is enabled and rows lacks {missing}")
        return True

    def th(name):
        return rules[name].astype(np.float64)[:, None]

    with np.errstate(invalid="ignore", over="ignore"):
        if need(BB_STATUS, "status"):
            c |= np.where((np.asarray(rows["status"]).astype(np.int32) & rules["status_mask"].astype(np.int32)[:, None]) != 0, BB_STATUS, 0).astype(np.int32)
        if need(BB_FALLBACK, "qp_iter"):
            c |= np.where(np.asarray(rows["qp_iter"]).astype(np.int64) // 1000 % 10 != 0, BB_FALLBACK, 0).astype(np.int32)
        if need(BB_NONFINITE, "x_odom", "w_odom", "cost_solution"):
            fin = np.isfinite(rows["x_odom"]).all(axis=2) & np.isfinite(rows["w_odom"]).all(axis=2) & np.isfinite(rows["cost_solution"])
            c |= np.where(~fin, BB_NONFINITE, 0).astype(np.int32)
        if need(BB_ERR_POS, "x_odom", "x_ref"):
            d = np.asarray(rows["x_odom"], dtype=np.float64)[:, :, 0:3] - np.asarray(rows["x_ref"], dtype=np.float64)[:, :, 0:3]
            s = (d[:, :, 0] * d[:, :, 0] + d[:, :, 1] * d[:, :, 1]) + d[:, :, 2] * d[:, :, 2]
            c |= np.where(s > th("err_pos") * th("err_pos"), BB_ERR_POS, 0).astype(np.int32)
        if need(BB_SPEED, "x_odom"):
            v = np.asarray(rows["x_odom"], dtype=np.float64)[:, :, 7:10]
            s = (v[:, :, 0] * v[:, :, 0] + v[:, :, 1] * v[:, :, 1]) + v[:, :, 2] * v[:, :, 2]
            c |= np.where(s > th("speed") * th("speed"), BB_SPEED, 0).astype(np.int32)
        if need(BB_TILT, "x_odom"):
            qx, qy = np.asarray(rows["x_odom"], dtype=np.float64)[:, :, 4], np.asarray(rows["x_odom"], dtype=np.float64)[:, :, 5]
            c |= np.where(1 - 2 * (qx * qx + qy * qy) < th("tilt_cos"), BB_TILT, 0).astype(np.int32)
        if need(BB_COST, "cost_solution"):
            c |= np.where(np.asarray(rows["cost_solution"], dtype=np.float64) > th("cost"), BB_COST, 0).astype(np.int32)
    return c & en

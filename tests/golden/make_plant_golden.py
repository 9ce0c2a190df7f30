#!/usr/bin/env python3
"""Generate tests/golden/plant_vectors.npz: the reference's own Quadrotor3D (src/quad.py) run on 128 randomised plants.

Runs only where the reference checkout is; the .npz it writes holds data only.  src/quad.py imports `utils.utils`, which cannot be
imported (dead imports, see make_golden.py): a stub module takes its place that holds the six functions quad.py uses, extracted from
src/utils/utils.py with ast and executed at generation time (the technique of make_golden.py's extract_utils_functions).

 * group 0 (cases 0..63):   20 x one_step_forward(x, u, 5e-3, f_d, t_d) with u in [0, 1] (the function asserts that range)
 * group 1 (cases 64..127): 20 x update(u, 5e-3) with u in [-0.2, 1.2] and no disturbance: update clips the input (src/quad.py:242-247)
Bases alternate between the legacy_sim and the hummingbird constants of mpc_quad_ros_amd/params.py; every parameter is drawn
independently (mass, each J, max_thrust, the arms of x_f and y_f, c, every drag coefficient x U(0.5, 2); z rotor drag + U(0, 0.2);
payload U(0, 0.3); functionality U(0, 1), all ones in a quarter of the cases; f_d N(0, 1); t_d N(0, 0.02)), so no two fields of a case are
equal.  States: position around hover, near-unit quaternion, v N(0, 4), r N(0, 0.5).  g = 9.81 (src/quad.py:73).
 * drag_v, drag_a [128, 3, M]: get_aero_drag(x, body_frame=True) of every plant at M states with q = [1, 0, 0, 0] and velocity drag_v.

Usage: python tests/golden/make_plant_golden.py [/root/reference]
"""
import ast
import os
import sys
import types

import numpy as np

REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
OUT = os.path.dirname(os.path.abspath(__file__))
NAMES = {"skew_symmetric", "quaternion_to_euler", "unit_quat", "v_dot_q", "quaternion_inverse", "q_to_rot_mat"}
NCASE, NSUB, DT, M = 128, 20, 5e-3, 6


def import_reference_quad():
    sys.dont_write_bytecode = True
    with open(os.path.join(REF, "src", "utils", "utils.py")) as fh:
        tree = ast.parse(fh.read())
    ns = {"np": np, "cs": types.SimpleNamespace(MX=type("MX", (), {}), SX=type("SX", (), {}))}
    for node in tree.body:
        if isinstance(node, ast.FunctionDef) and node.name in NAMES:
            exec(compile(ast.Module(body=[node], type_ignores=[]), "utils_extract", "exec"), ns)
    pkg, mod = types.ModuleType("utils"), types.ModuleType("utils.utils")
    for n in NAMES:
        setattr(mod, n, ns[n])
    mod.parse_xacro_file = lambda *a, **k: None
    sys.modules["utils"], sys.modules["utils.utils"] = pkg, mod
    sys.path.insert(0, os.path.join(REF, "src"))
    from quad import Quadrotor3D
    return Quadrotor3D


def main():
    Quadrotor3D = import_reference_quad()
    rng = np.random.default_rng(20240611)
    # (mass, J, max_thrust, arm, c, sign of z_l_tau): legacy_sim() and hummingbird() of mpc_quad_ros_amd/params.py
    bases = [(1.0, (0.03, 0.03, 0.06), 20.0, 0.47 / 2, 0.013, 1.0),
             (0.68 + 4 * 0.009, (0.007, 0.007, 0.012), 838.0 ** 2 * 8.54858e-06, 0.17, 0.016, -1.0)]
    s = lambda n=None: rng.uniform(0.5, 2.0, n)
    out = {k: [] for k in ("mass", "J", "max_thrust", "x_f", "y_f", "z_l_tau", "rotor_drag", "aero_drag", "payload_mass", "rotor_functionality",
                           "f_d", "t_d", "x0", "u", "x_ref", "group", "base", "drag_v", "drag_a")}
    for case in range(NCASE):
        mass, J, tmax, arm, c, sgn = bases[case % 2]
        group = case // (NCASE // 2)
        q = Quadrotor3D(payload=True, drag=True)
        q.mass, q.J, q.max_thrust = mass * s(), np.array(J) * s(3), tmax * s()
        q.x_f = np.array([1.0, 0, -1.0, 0]) * arm * s()
        q.y_f = np.array([0, 1.0, 0, -1.0]) * arm * s()
        q.z_l_tau = sgn * np.array([-1.0, 1.0, -1.0, 1.0]) * c * s()
        q.rotor_drag = np.array([0.3, 0.3, 0.0]) * s(3) + np.array([0, 0, rng.uniform(0, 0.2)])
        q.aero_drag = 0.008 * s()
        q.payload_mass = rng.uniform(0, 0.3)
        q.rotor_functionality = rng.uniform(0, 1, 4) if case % 4 else np.ones(4)
        f_d, t_d = rng.normal(0, 1.0, 3), rng.normal(0, 0.02, 3)
        x0 = np.zeros(13)
        x0[0:3] = rng.normal(0, 2.0, 3) + np.array([0, 0, 3.0])
        qq = rng.normal(0, 0.25, 4) + np.array([1.0, 0, 0, 0])
        x0[3:7] = qq / np.linalg.norm(qq)
        x0[7:10], x0[10:13] = rng.normal(0, 4.0, 3), rng.normal(0, 0.5, 3)
        if group == 0:
            u = rng.uniform(0, 1, 4)
            x = x0.copy()
            for _ in range(NSUB):
                x = q.one_step_forward(x, u, DT, f_d, t_d)
        else:
            u = rng.uniform(-0.2, 1.2, 4)
            f_d, t_d = np.zeros(3), np.zeros(3)
            q.set_state(x0.copy())
            for _ in range(NSUB):
                q.update(u.copy(), DT)
            x = q.get_state(quaternion=True, stacked=True)
        vs = rng.normal(0, 5.0, (M, 3))
        drag = []
        for v in vs:
            xs = np.zeros(13)
            xs[3], xs[7:10] = 1.0, v
            drag.append(np.asarray(q.get_aero_drag(xs, body_frame=True), dtype=np.float64))
        for k, v in (("mass", q.mass), ("J", q.J), ("max_thrust", q.max_thrust), ("x_f", q.x_f), ("y_f", q.y_f), ("z_l_tau", q.z_l_tau),
                     ("rotor_drag", q.rotor_drag), ("aero_drag", q.aero_drag), ("payload_mass", q.payload_mass),
                     ("rotor_functionality", q.rotor_functionality), ("f_d", f_d), ("t_d", t_d), ("x0", x0), ("u", u), ("x_ref", x),
                     ("group", group), ("base", case % 2), ("drag_v", vs.T), ("drag_a", np.array(drag).T)):
            out[k].append(np.array(v, dtype=np.float64))
    res = {k: np.array(v) for k, v in out.items()}
    res["group"], res["base"] = res["group"].astype(np.int32), res["base"].astype(np.int32)
    res["g"], res["sim_dt"], res["n_sub"] = np.float64(9.81), np.float64(DT), np.int32(NSUB)
    res["source"] = "src/quad.py Quadrotor3D(payload=True, drag=True): one_step_forward / update / get_aero_drag"
    np.savez_compressed(os.path.join(OUT, "plant_vectors.npz"), **res)
    print("wrote plant_vectors.npz:", {k: v.shape for k, v in res.items() if hasattr(v, "shape") and v.shape})


if __name__ == "__main__":
    main()

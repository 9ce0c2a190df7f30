#!/usr/bin/env python3
"""Generate tests/golden/explore_vectors.npz: the reference's own exploration rule (src/Explorer.py) on random envelopes.

Runs only where the reference checkout is; the .npz it writes holds data only.  src/Explorer.py imports plotting packages at module
level, so the two methods of the rule -- calculate_explored_vmax (:51-63) and calculate_velocity_to_explore (:40-48) -- are extracted
with ast and executed at generation time on a stand-in for `self` that carries exploration_step and desired_explored_vmax (the
technique of make_golden.py's extract_utils_functions).

 * env [n, 3, 2]: min and max per axis, step [n], desired [n] -> explored [n], velocity [n]
 * cases 0..15 are made by hand: the all-zero envelope (Explorer's `gpe is None`), ties between two and three axes, an axis that never left
   zero, negative reach larger than the positive one, a max below zero, and explored + step == desired exactly (the `<` is strict);
   the rest is random: reach per axis U(0, 25) on either side, a quarter of the cases with the reference's step 10 / desired 20, every
   eighth random case with desired = explored + step exactly.

Usage: python tests/golden/make_explore_golden.py [/root/reference]
"""
import ast
import os
import sys
import types

import numpy as np

REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
OUT = os.path.dirname(os.path.abspath(__file__))
NAMES = ("calculate_explored_vmax", "calculate_velocity_to_explore")
NRANDOM = 384


def extract_rule():
    with open(os.path.join(REF, "src", "Explorer.py")) as fh:
        tree = ast.parse(fh.read())
    cls = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "Explorer")
    ns = {}
    for node in cls.body:
        if isinstance(node, ast.FunctionDef) and node.name in NAMES:
            exec(compile(ast.Module(body=[node], type_ignores=[]), "explorer_extract", "exec"), ns)
    return [ns[n] for n in NAMES]


def main():
    explored_vmax, velocity_to_explore = extract_rule()
    rng = np.random.default_rng(20240923)
    hand = [  # (env [3][2], step, desired)
        ([[0, 0], [0, 0], [0, 0]], 10.0, 20.0),
        ([[0, 0], [0, 0], [0, 0]], 1.5, 1.0),
        ([[-3.0, 3.0], [-3.0, 3.0], [-1.0, 3.0]], 10.0, 20.0),
        ([[-2.0, 5.0], [-5.0, 2.0], [-7.0, 1.0]], 10.0, 20.0),
        ([[-4.0, 4.0], [-6.0, 4.0], [-9.0, 9.5]], 2.0, 30.0),
        ([[-8.0, 7.0], [0.0, 0.0], [-1.0, 2.0]], 10.0, 20.0),
        ([[-12.5, 3.0], [-11.0, 2.0], [-13.0, 1.0]], 10.0, 20.0),
        ([[-6.0, -1.0], [-7.0, -2.0], [-8.0, -3.0]], 1.0, 9.0),
        ([[1.0, 6.0], [2.0, 7.0], [3.0, 8.0]], 1.0, 9.0),
        ([[-10.0, 10.0], [-10.0, 12.0], [-11.0, 10.0]], 10.0, 20.0),       # explored + step == desired
        ([[-2.5, 2.0], [-3.0, 2.5], [-2.5, 2.5]], 1.25, 3.75),            # the same with binary fractions
        ([[-0.75, 0.5], [-1.0, 0.75], [-0.75, 0.25]], 0.5, 1.25),
        ([[-9.0, 9.0], [-9.0, 9.0], [-9.0, 9.0]], 10.0, 19.0),
        ([[-9.0, 9.0], [-9.0, 9.0], [-9.0, 9.0]], 10.0, 19.000000000000004),
        ([[-25.0, 25.0], [-26.0, 24.0], [-30.0, 31.0]], 10.0, 20.0),
        ([[-1e-300, 0.0], [-5.0, 5.0], [-5.0, 5.0]], 10.0, 20.0),
    ]
    env, step, desired = [np.array(h[0], dtype=np.float64) for h in hand], [h[1] for h in hand], [h[2] for h in hand]
    for k in range(NRANDOM):
        e = np.stack([-rng.uniform(0, 25, 3), rng.uniform(0, 25, 3)], axis=1)
        if k % 5 == 0:                      # a one-sided axis
            e[rng.integers(3), rng.integers(2)] *= -0.3
            e = np.sort(e, axis=1)
        if k % 7 == 0:                      # a tie between two axes
            i, j = rng.choice(3, 2, replace=False)
            e[j] = e[i]
        s, d = (10.0, 20.0) if k % 4 == 0 else (rng.uniform(0.5, 12.0), rng.uniform(0.5, 40.0))
        env.append(e); step.append(s); desired.append(d)
    env, step, desired = np.array(env), np.array(step), np.array(desired)
    explored = np.zeros(len(env))
    for k in range(len(env)):
        explored[k] = explored_vmax(None, [{"min": float(a[0]), "max": float(a[1])} for a in env[k]])
    for k in range(16 + 3, len(env), 8):    # explored + step == desired exactly, as the sum the rule forms
        desired[k] = explored[k] + step[k]
    velocity = np.zeros(len(env))
    for k in range(len(env)):
        me = types.SimpleNamespace(exploration_step=float(step[k]), desired_explored_vmax=float(desired[k]))
        velocity[k] = velocity_to_explore(me, float(explored[k]))
    exact = explored + step == desired
    assert exact.sum() >= 40 and (velocity[exact] == desired[exact]).all()
    assert (velocity < desired).any() and (velocity == desired).any() and (explored[:2] == 0).all()
    np.savez_compressed(os.path.join(OUT, "explore_vectors.npz"), env=env, step=step, desired=desired, explored=explored, velocity=velocity,
                        source="src/Explorer.py calculate_explored_vmax / calculate_velocity_to_explore")
    print("wrote explore_vectors.npz:", len(env), "cases,", int(exact.sum()), "with explored + step == desired,",
          int((velocity < desired).sum()), "below desired")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Generate tests/golden/rgp_predict_vectors.npz: posterior mean / variance / standard deviation of the reference's recursive GP
(src/gp/RGP.py:168-229, numpy path) and static GP (src/gp/GP.py:135-179) at query points, arrays only.

Runs only where the reference checkout is; the tests read the .npz and nothing else.  The reference modules are imported the way
make_golden.py imports them (casadi stubbed: only the numpy path executes).

* r{c}_{K}_*: the six (nb, theta, v_max) cases of rgp_vectors.npz after K in {0, 25, 300} regressed samples of a seeded stream:
  X, theta, mu, C, xq, mean, var (diagonal of cov=True), std.
* s{c}_*: the three static cases of gp_vectors.npz (same X, y, theta): xq, mean, var of GP.predict.
Query points: np.arange(-20, 20, 0.5) plus 16 seeded points within +-1.5 v_max (static: +-15).

Usage: python tests/golden/make_predict_golden.py [reference checkout]
"""
import os
import sys

import numpy as np

sys.argv = sys.argv[:2]
from make_golden import OUT, REF, import_reference_rgp   # noqa: E402

RGP_CASES = [(10, [1.0, 0.1, 0.1], 12.0), (10, [3.0, 0.1, 0.01], 10.0), (20, [1.0, 1.0, 0.1], 10.0),
             (50, [1.0, 0.1, 0.1], 12.0), (20, [1.0, 0.1, 0.1], 12.0), (10, [3.0, 0.5, 0.01], 15.0)]      # make_golden.make_rgp_vectors
KS = (0, 25, 300)
GRID = np.arange(-20, 20, 0.5)


def main():
    ref = import_reference_rgp()
    sys.path.insert(0, os.path.join(REF, "src", "gp"))
    import GP as ref_gp  # noqa
    rng = np.random.default_rng(20261016)
    out = {}
    for ci, (nb, theta, vmax) in enumerate(RGP_CASES):
        X = np.linspace(-vmax, vmax, nb)
        for K in KS:
            g = ref.RGP(X, np.zeros(nb), theta=list(theta))
            s = rng.uniform(-1.2 * vmax, 1.2 * vmax, K)
            y = 0.3 * s + 0.02 * s * np.abs(s) + rng.normal(0, 0.5, K)
            for k in range(K):
                g.regress(np.array([s[k]]), np.array([y[k]]))
            xq = np.concatenate([GRID, rng.uniform(-1.5 * vmax, 1.5 * vmax, 16)])
            mean, cov = g.predict(xq, cov=True)
            mean_s, std = g.predict(xq, std=True)
            assert np.array_equal(mean, mean_s)
            p = f"r{ci}_{K}_"
            out[p + "X"] = X; out[p + "theta"] = np.array(theta, dtype=np.float64)
            out[p + "mu"] = np.array(g.mu_g_t, dtype=np.float64).ravel(); out[p + "C"] = np.array(g.C_g_t, dtype=np.float64)
            out[p + "xq"] = xq; out[p + "mean"] = np.array(mean, dtype=np.float64).ravel()
            out[p + "var"] = np.diag(cov).astype(np.float64); out[p + "std"] = np.array(std, dtype=np.float64).ravel()
    gv = np.load(os.path.join(OUT, "gp_vectors.npz"))
    for ci in range(int(gv["ncases"])):
        X, y, theta = gv[f"c{ci}_X"], gv[f"c{ci}_y"], gv[f"c{ci}_theta"]
        g = ref_gp.GP(X, y, theta=list(theta))
        xq = np.concatenate([GRID, rng.uniform(-15, 15, 16)])
        mean, var = g.predict(xq, var=True)
        p = f"s{ci}_"
        out[p + "xq"] = xq; out[p + "mean"] = np.array(mean, dtype=np.float64).ravel(); out[p + "var"] = np.array(var, dtype=np.float64).ravel()
    out["n_rgp"] = len(RGP_CASES); out["n_static"] = int(gv["ncases"]); out["Ks"] = np.array(KS)
    np.savez_compressed(os.path.join(OUT, "rgp_predict_vectors.npz"), **out)
    vmin = min(out[k].min() for k in out if k.endswith("_var"))
    print("wrote rgp_predict_vectors.npz", os.path.getsize(os.path.join(OUT, "rgp_predict_vectors.npz")), "bytes; smallest reference variance", vmin)


if __name__ == "__main__":
    main()

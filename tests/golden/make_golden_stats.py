#!/usr/bin/env python3
"""Generate tests/golden/g21_stats.npz from the reference: Cramer-Rao bounds and confidence intervals (epgpy/stats.py).

Run ONLY in the build container, where the upstream reference (py-baudin/epgpy) is mounted read-only:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_stats.py

As make_golden.py: the reference is imported as a black box and driven through its public API; only the resulting data
(inputs and expected outputs) are written.

Cases (G21), a few voxels x <= 12 points x <= 5 parameters, seeded complex Gaussian inputs:
  crlb     J [3, 2, 12, 5]: plain; with W (a vector), sigma2 = 0.3 and log; with W that varies over the voxels
  grad     J [4, 10, 3], H [4, 10, 3, 2]: (cost, grad) plain and with W / sigma2 / log
  split    crlb_split of the first J: plain; with W, sigma2 and log
  confint  obs / pred [4, 12], jac [4, 12, 2] with and without hess [4, 12, 2, 2], conflevel 0.99 and 0.8 at 10 degrees of
           freedom.  The t value is a factor of every output, so the cases lie where the reference's t value (its built-in
           table for dof 1 .. 99 at 0.95 and 1 .. 9 at 0.99, scipy outside it) agrees with the product's computed quantile well
           inside the 1e-12 of the golden comparison: elsewhere that comparison would measure the t values, not the formulas.
           (The quantile of the product is tested on its own, tests/test_stats_host.py.)
"""
import os
import sys

sys.dont_write_bytecode = True
REFERENCE = os.environ.get("EPGPY_REFERENCE", "/root/reference")
sys.path.insert(0, REFERENCE)

import numpy as np  # noqa: E402

if not hasattr(np, "asfarray"):      # (NumPy 2 removed it; the reference's spline helper still calls it)
    np.asfarray = lambda a: np.asarray(a, dtype=np.float64)

from epgpy import stats  # noqa: E402  (the reference)

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = {}


def put(name, value):
    OUT[name] = np.asarray(value)


def cgauss(rng, *shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


rng = np.random.default_rng(21)

# ------------------------------------------------------------------------------------------------------------ crlb / split
J = cgauss(rng, 3, 2, 12, 5)
W = np.array([1.0, 0.5, 2.0, 0.0, 3.0])
Wmap = rng.uniform(0.5, 2.0, (3, 2, 5))
put("crlb_J", J)
put("crlb_W", W)
put("crlb_Wmap", Wmap)
put("crlb_plain", stats.crlb(J))
put("crlb_w_log", stats.crlb(J, W=W, sigma2=0.3, log=True))
put("crlb_wmap", stats.crlb(J, W=Wmap))
put("split_plain", stats.crlb_split(J))
put("split_w_log", stats.crlb_split(J, W=W[[0, 1, 2, 4, 4]], sigma2=0.3, log=True))

# ------------------------------------------------------------------------------------------------------------ gradient
Jg, Hg = cgauss(rng, 4, 10, 3), cgauss(rng, 4, 10, 3, 2)
Wg = np.array([2.0, 1.0, 0.25])
put("grad_J", Jg)
put("grad_H", Hg)
put("grad_W", Wg)
cost, grad = stats.crlb(Jg, Hg)
put("grad_cost", cost)
put("grad_grad", grad)
cost, grad = stats.crlb(Jg, Hg, W=Wg, sigma2=1.7, log=True)
put("grad_cost_w_log", cost)
put("grad_grad_w_log", grad)

# ------------------------------------------------------------------------------------------------------------ confint
jac, hess = cgauss(rng, 4, 12, 2), 0.05 * cgauss(rng, 4, 12, 2, 2)
pred = cgauss(rng, 4, 12)
obs = pred + 0.1 * cgauss(rng, 4, 12)
put("ci_obs", obs)
put("ci_pred", pred)
put("ci_jac", jac)
put("ci_hess", hess)
for level in (0.99, 0.8):
    tag = str(level).replace("0.", "")
    cints, cband = stats.confint(obs, pred, jac, conflevel=level)
    put(f"ci_cints_{tag}", cints)
    put(f"ci_cband_{tag}", cband)
    cints, cband = stats.confint(obs, pred, jac, hess, conflevel=level)
    put(f"ci_cints_hess_{tag}", cints)
    put(f"ci_cband_hess_{tag}", cband)

path = os.path.join(HERE, "g21_stats.npz")
np.savez_compressed(path, **OUT)
print(f"wrote {path}: {len(OUT)} arrays, {os.path.getsize(path)} bytes")

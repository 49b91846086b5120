"""Cramer-Rao bounds of a two-pool exchange experiment: an RF-spoiled gradient echo with exchange between a free and a bound
pool (epg.X), differentiated on the GPU with respect to the exchange rate, the bound pool's T1 (at fixed pool fractions) and
B1 (a common scale of the flip angles).  The receiver sees the sum of the pools, so the Jacobian is summed over the
compartment axis before the bounds are taken (epgpy_amd.stats.crlb on the host).

    python examples/exchange_crlb.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from epgpy_amd import epg, exchange, stats  # noqa: E402

NTR, TR = 40, 8.0
fractions = np.array([0.85, 0.15])                  # free pool, bound pool
k, T1, T2 = 0.03, np.array([1000.0, 350.0]), np.array([70.0, 12.0])
alphas = 5.0 + 30.0 * np.sin(np.linspace(0, np.pi, NTR)) ** 2       # a flip-angle schedule to compare against a constant one

direction = exchange.exchange_matrix(1.0, densities=fractions)      # d khi / d k at fixed pool fractions


def sequence(flip):
    x = epg.X(TR, k * direction, T1=T1, T2=T2, dkhi=direction,
              order1={"k": {"khi": 1}, "T1b": {"T1": [0.0, 1.0]}})
    seq = [epg.PD(fractions)]
    for j in range(NTR):
        seq += [epg.T(flip[j], 58.5 * j * (j + 1), order1={"B1": {"alpha": flip[j]}}), epg.ADC, x, epg.S(1)]
    return seq


variables = ["k", "T1b", "B1"]
for name, flip in (("constant 20 deg", np.full(NTR, 20.0)), ("sin^2 schedule", alphas)):
    jac = epg.simulate(sequence(flip), probe=epg.Jacobian(["magnitude"] + variables))      # [NTR, 2 pools, 1 + 3]
    total = jac.sum(axis=1)                                                             # what the receiver sees
    bound = stats.crlb(total[..., 1:], sigma2=1e-6)
    print(f"{name}: signal of the first echoes {np.abs(total[:3, 0]).round(4)}")
    print(f"  Cramer-Rao bound (sum of variances of {variables}): {float(np.asarray(bound)):.4g}")

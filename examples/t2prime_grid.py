"""A gradient-echo decay over a (T2, T2') grid in one call: the time accumulation C with one R2' per grid row.

    python examples/t2prime_grid.py

C(tau, R2') moves every voxel's rows along the time coordinate by its own tau * R2': the coordinate sets differ between the
voxels, which the option voxel_coords=True runs per voxel on the device.  ADC weighs the rows of each voxel with
exp(-|t|): a Lorentzian line of width R2' gives the free-induction decay exp(-t / T2) exp(-t R2') = exp(-t / T2*).
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from epgpy_amd import epg  # noqa: E402

T2 = np.array([40.0, 80.0, 120.0, 200.0])          # ms, along the second grid axis
R2p = np.array([0.005, 0.02, 0.05])                # 1/ms (T2' = 200, 50, 20 ms), along the first
tau, necho = 2.0, 12                               # ms between the echoes

seq = [epg.T(90, 90)] + [epg.E(tau, 1e9, T2[None, :]), epg.C(tau, R2p[:, None]), epg.ADC] * necho
signal = np.abs(epg.simulate(seq, kgrid=1e-3, voxel_coords=True))          # [necho, 3, 4]

t = tau * np.arange(1, necho + 1)
expected = np.exp(-t[:, None, None] * (1.0 / T2[None, None, :] + R2p[None, :, None]))
print("largest deviation from exp(-t / T2*):", np.abs(signal - expected).max())
for i, r in enumerate(R2p):
    for j, t2 in enumerate(T2):
        fit = -np.polyfit(t, np.log(signal[:, i, j]), 1)[0]
        print(f"T2 = {t2:5.0f} ms, T2' = {1 / r:5.0f} ms: T2* fitted {1 / fit:6.2f} ms, expected {1 / (1 / t2 + r):6.2f} ms")
assert np.abs(signal - expected).max() < 1e-9

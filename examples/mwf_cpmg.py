"""Myelin water fraction from a multi-echo CPMG train: every voxel as a NON-NEGATIVE MIXTURE of the T2 atoms of an EPG dictionary.

`simulate(..., out="device")` leaves a 32-echo dictionary over (T2 x B1) in HBM -- EPG, so that the stimulated echoes of an
imperfect refocusing pulse are part of every atom.  `match.Components` takes the T2 axis as the component axis and computes the
Gram matrices of every B1 next to the records; `match.nnls` fits the T2 spectrum of every voxel at every B1 on the device and keeps
the B1 of the best fit; the myelin water fraction is the share of the spectrum below 40 ms.  With `chi2=1.02` the same call then
raises the Tikhonov weight of every voxel on the device until the data misfit has grown by 2 % (the discrepancy principle of
Whittall and MacKay) and returns the smooth spectrum; over repeated noise draws of ONE voxel the spiky plain spectrum and the
regularised one are compared by the spread of MWF and of the geometric mean T2.

    python examples/mwf_cpmg.py [n_T2] [n_B1] [nvoxel]      # defaults 40, 16, 2000
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))   # run from a checkout
from epgpy_amd import epg, match  # noqa: E402

n2 = int(sys.argv[1]) if len(sys.argv) > 1 else 40
nb = int(sys.argv[2]) if len(sys.argv) > 2 else 16
nvox = int(sys.argv[3]) if len(sys.argv) > 3 else 2000

NECHO, ESP, T1 = 32, 10.0, 1000.0                                        # echoes, echo spacing and T1 in ms


def cpmg(T2, B1):
    rlx = epg.E(ESP / 2, T1, T2)
    return [epg.T(90, 90)] + [epg.S(1), rlx, epg.T(180.0 * B1, 0), epg.S(1), rlx, epg.ADC] * NECHO


T2_grid = np.geomspace(10.0, 2000.0, n2)
B1_grid = np.linspace(0.7, 1.0, nb)
dictionary = epg.simulate(cpmg(T2_grid[:, None], B1_grid[None, :]), out="device")      # [32, n2, nb] in HBM
components = match.Components(dictionary, axis=0)                                     # H_g of every B1, once

# two pools per voxel: myelin water at 20 ms, intra- and extracellular water at 80 ms, at a B1 of the grid
rng = np.random.default_rng(2024)
mwf_true = rng.uniform(0.05, 0.25, nvox)
b1_index = rng.integers(0, nb, nvox)
b1_true = B1_grid[b1_index]
signals = mwf_true * np.asarray(epg.simulate(cpmg(20.0, b1_true))) + (1 - mwf_true) * np.asarray(epg.simulate(cpmg(80.0, b1_true)))
sigma = 1e-3
signals = signals + sigma * (rng.standard_normal(signals.shape) + 1j * rng.standard_normal(signals.shape))

fit = match.nnls(components, signals)                                   # weights [n2, nvox], group = the B1 index
mwf = fit.fraction(0.0, 40.0, T2_grid)
(b1_found,) = fit.unravel()

print(f"{NECHO} echoes, dictionary {n2} x {nb} (T2 x B1) on the device, {nvox} two-pool voxels, noise sigma {sigma:g}")
print(f"    B1 recovered within one grid step in {np.mean(np.abs(b1_found - b1_index) <= 1) * 100:.1f} % of the voxels")
print(f"    myelin water fraction: true 0.05 .. 0.25, error median {np.nanmedian(np.abs(mwf - mwf_true)):.4f}, "
      f"95th percentile {np.nanpercentile(np.abs(mwf - mwf_true), 95):.4f}")
print(f"    geometric mean T2: median {np.nanmedian(fit.gmean(T2_grid)):.1f} ms;  atoms with weight: median "
      f"{int(np.median((fit.weights > 0).sum(axis=0)))};  status 0 / 1 / 2: {np.bincount(fit.status, minlength=3).tolist()}")

# the regularised fit next to the plain one: one voxel (MWF 0.15, B1 of the grid's middle), `ndraw` noise draws
ndraw = 200
clean = 0.15 * np.asarray(epg.simulate(cpmg(20.0, B1_grid[nb // 2]))) + 0.85 * np.asarray(epg.simulate(cpmg(80.0, B1_grid[nb // 2])))
draws = clean.reshape(NECHO, 1) + sigma * (rng.standard_normal((NECHO, ndraw)) + 1j * rng.standard_normal((NECHO, ndraw)))
print(f"    one voxel (MWF 0.15), {ndraw} noise draws:          MWF mean +- sd        gmean T2 mean +- sd     atoms   status 0 .. 4")
for name, kw in (("plain", {}), ("chi2 = 1.02", dict(chi2=1.02))):
    f = match.nnls(components, draws, **kw)
    m, gm = f.fraction(0.0, 40.0, T2_grid), f.gmean(T2_grid)
    print(f"        {name:12s}                              {np.nanmean(m):.4f} +- {np.nanstd(m):.4f}      {np.nanmean(gm):6.1f} +- {np.nanstd(gm):4.1f} ms"
          f"      {int(np.median((f.weights > 0).sum(axis=0))):3d}     {np.bincount(f.status, minlength=5).tolist()}")

"""MR fingerprinting off the grid: a COARSE (T1, T2) dictionary with its Jacobian left on the GPU, a match against it, and one
Gauss-Newton step from the matched atom that uses the derivative rows where they lie.

`simulate(..., probe=epg.Jacobian([...]), out="device")` leaves fingerprints and their T1 / T2 derivatives in HBM;
`match.match` finds the best grid point of every voxel, `match.refine` moves it between the grid points (8 bytes per voxel go up,
8 P + 24 come back), `estimate` adds the step to the grid values.  A coarse dictionary then resolves what a fine one would.

    python examples/mrf_match_refine.py [n_T1] [n_T2] [ntr] [nvoxel]      # defaults 24, 24, 200, 1000
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))   # run from a checkout
from epgpy_amd import epg, match  # noqa: E402

n1 = int(sys.argv[1]) if len(sys.argv) > 1 else 24
n2 = int(sys.argv[2]) if len(sys.argv) > 2 else 24
ntr = int(sys.argv[3]) if len(sys.argv) > 3 else 200
nvox = int(sys.argv[4]) if len(sys.argv) > 4 else 1000

TR, TE = 12.0, 3.0                                                       # ms
angles = 10.0 + 50.0 * np.abs(np.sin(np.pi * np.arange(ntr) / 100.0))    # degrees


def train(T1, T2, **kw):
    seq = [epg.T(180, 0), epg.E(20.0, T1, T2, **kw), epg.SPOILER]
    for alpha in angles:
        seq += [epg.T(alpha, 90), epg.E(TE, T1, T2, **kw), epg.ADC, epg.E(TR - TE, T1, T2, **kw), epg.S(1)]
    return seq


T1_grid = np.geomspace(300.0, 3000.0, n1)[:, None]
T2_grid = np.geomspace(20.0, 300.0, n2)[None, :]
jac = epg.simulate(train(T1_grid, T2_grid, order1=["T1", "T2"]), probe=epg.Jacobian(["magnitude", "T1", "T2"]), max_nstate=63,
                   out="device")                                         # [ntr, n1, n2, 3] in HBM
dictionary = match.Dictionary(jac)                                       # its probed-state row, with the norms

rng = np.random.default_rng(2024)
T1_true = rng.uniform(400.0, 2500.0, nvox)
T2_true = rng.uniform(30.0, 250.0, nvox)
density = (0.5 + rng.random(nvox)) * np.exp(2j * np.pi * rng.random(nvox))
sigma = 0.002
signals = np.asarray(epg.simulate(train(T1_true, T2_true), max_nstate=63)) * density
signals = signals + sigma * (rng.standard_normal(signals.shape) + 1j * rng.standard_normal(signals.shape))

res = match.match(dictionary, signals)
# one step in T1 and T2, at most one grid spacing long
limit = [T1_grid.max() * (T1_grid[1, 0] / T1_grid[0, 0] - 1), T2_grid.max() * (T2_grid[0, 1] / T2_grid[0, 0] - 1)]
ref = match.refine(dictionary, signals, res, variables=["T1", "T2"], limit=limit)
est = ref.estimate([T1_grid, T2_grid])                                   # [nvox, 2]

i1, i2 = res.unravel()
print(f"{ntr} TR, dictionary {n1} x {n2} (T1 x T2) with its Jacobian on the device, {nvox} voxels, noise sigma {sigma:g}")
for name, grid, hat, fine, true in (("T1", T1_grid[1, 0] / T1_grid[0, 0], T1_grid[i1, 0], est[:, 0], T1_true),
                                    ("T2", T2_grid[0, 1] / T2_grid[0, 0], T2_grid[0, i2], est[:, 1], T2_true)):
    e0, e1 = np.abs(hat / true - 1) * 100, np.abs(fine / true - 1) * 100
    print(f"    {name}: grid spacing {(grid - 1) * 100:.1f} %; matched within median {np.median(e0):.2f} % (95th percentile "
          f"{np.percentile(e0, 95):.2f} %), refined within {np.nanmedian(e1):.2f} % ({np.nanpercentile(e1, 95):.2f} %)")
print(f"    unresolved voxels: {int(np.isnan(ref.delta).any(axis=1).sum())};  score: median {np.median(res.score):.6f} -> "
      f"{np.median(ref.score):.6f}")

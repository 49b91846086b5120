"""MR fingerprinting in three steps that all stay on the GPU: simulate a dictionary over a (T1, T2) grid, compress it onto
its leading singular vectors (`match.compress`), then match measured signals in the compressed space.  This is
examples/mrf_match.py with the `compress` step: the Gram matrix of the fingerprints [ntr, ntr] comes down, its eigenvectors
go up, and dictionary and signals are projected on the device -- matching then runs at `rank` records instead of `ntr`.

The dictionary never leaves the device: `simulate(..., out="device")` leaves the fingerprints in HBM, `match.Dictionary` adds
their norms there, and `match.match` returns per voxel the best grid point, the complex proton density and the correlation --
32 bytes per voxel.

The train: an inversion, then `ntr` excitations with a slowly varying flip angle and a gradient spoiler per TR (FISP-like).
The phantom: voxels at OFF-grid (T1, T2) with a complex density and seeded Gaussian noise.

    python examples/mrf_match_compressed.py [n_T1] [n_T2] [ntr] [nvoxel] [energy] [dtype]  # defaults 64, 64, 200, 1000, 0.99999, complex128

With dtype `complex64` the compressed dictionary is kept in single precision (`compress(..., dtype=np.complex64)`: the projected
dictionary rounded once, half the bytes) and matched on the fp32 matrix cores; one more line then compares it with the
complex128 match.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))   # run from a checkout
from epgpy_amd import epg, match  # noqa: E402

n1 = int(sys.argv[1]) if len(sys.argv) > 1 else 64
n2 = int(sys.argv[2]) if len(sys.argv) > 2 else 64
ntr = int(sys.argv[3]) if len(sys.argv) > 3 else 200
nvox = int(sys.argv[4]) if len(sys.argv) > 4 else 1000
energy = float(sys.argv[5]) if len(sys.argv) > 5 else 0.99999
dtype = np.dtype(sys.argv[6]) if len(sys.argv) > 6 else np.dtype(np.complex128)

TR, TE = 12.0, 3.0                                                       # ms
angles = 10.0 + 50.0 * np.abs(np.sin(np.pi * np.arange(ntr) / 100.0))    # degrees


def train(T1, T2):
    seq = [epg.T(180, 0), epg.E(20.0, T1, T2), epg.SPOILER]
    for alpha in angles:
        seq += [epg.T(alpha, 90), epg.E(TE, T1, T2), epg.ADC, epg.E(TR - TE, T1, T2), epg.S(1)]
    return seq


T1_grid = np.geomspace(300.0, 3000.0, n1)
T2_grid = np.geomspace(20.0, 300.0, n2)
fingerprints = epg.simulate(train(T1_grid[:, None], T2_grid[None, :]), max_nstate=63, out="device")     # [ntr, n1, n2] in HBM
dictionary = match.Dictionary(fingerprints)
basis = match.compress(dictionary, energy=energy)             # basis.dictionary: [rank, n1, n2] in HBM

rng = np.random.default_rng(2024)
T1_true = rng.uniform(400.0, 2500.0, nvox)
T2_true = rng.uniform(30.0, 250.0, nvox)
density = (0.5 + rng.random(nvox)) * np.exp(2j * np.pi * rng.random(nvox))
sigma = 0.002
signals = np.asarray(epg.simulate(train(T1_true, T2_true), max_nstate=63)) * density
signals = signals + sigma * (rng.standard_normal(signals.shape) + 1j * rng.standard_normal(signals.shape))

res = match.match(basis.dictionary, signals)                   # the signals are projected on the device, then matched
full = match.match(dictionary, signals)
i1, i2 = res.unravel()
T1_hat, T2_hat = T1_grid[i1], T2_grid[i2]
step1, step2 = (T1_grid[1] / T1_grid[0] - 1) * 100, (T2_grid[1] / T2_grid[0] - 1) * 100
err1, err2 = np.abs(T1_hat / T1_true - 1) * 100, np.abs(T2_hat / T2_true - 1) * 100
print(f"{ntr} TR, dictionary {n1} x {n2} (T1 x T2) on the device, {nvox} voxels, noise sigma {sigma:g}")
print(f"    T1: grid spacing {step1:.1f} %, matched within median {np.median(err1):.1f} %, 95th percentile {np.percentile(err1, 95):.1f} %")
print(f"    T2: grid spacing {step2:.1f} %, matched within median {np.median(err2):.1f} %, 95th percentile {np.percentile(err2, 95):.1f} %")
print(f"    rank {basis.rank} of {basis.nrec} records keeps {basis.energy:.8f} of the energy; "
      f"{np.mean(res.index == full.index) * 100:.1f} % of the voxels get the atom of the uncompressed match")
print(f"    density: median |scale / true - 1| = {np.median(np.abs(res.scale / density - 1)):.3f};  score: median {np.median(res.score):.5f}")
if dtype == np.complex64:
    single = match.match(match.compress(dictionary, energy=energy, dtype=np.complex64).dictionary, signals)
    print(f"    complex64 compressed dictionary ({8 * basis.rank * n1 * n2} bytes): {np.mean(single.index == res.index) * 100:.1f} % of the voxels "
          f"get the atom of the complex128 match; largest |scale - scale128| = {np.max(np.abs(single.scale - res.scale)):.2e}")

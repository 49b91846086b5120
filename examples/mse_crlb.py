"""How precisely can a multi-spin-echo train measure T2?  Cramer-Rao lower bound of T2 over a grid of echo spacings and T2
values, once with T2 as the only unknown and once with the signal magnitude unknown as well -- the usual fit.

The Jacobian never leaves the GPU: `simulate(..., probe=epg.Jacobian([...]), out="device")` leaves signal and derivative in
HBM, `stats.crlb` reads them there, and what comes back is the map, 8 bytes per grid point.

    python examples/mse_crlb.py [n_spacing] [n_T2] [necho]      # defaults 48, 64, 16
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))   # run from a checkout
from epgpy_amd import epg, stats  # noqa: E402

ns = int(sys.argv[1]) if len(sys.argv) > 1 else 48
nt = int(sys.argv[2]) if len(sys.argv) > 2 else 64
necho = int(sys.argv[3]) if len(sys.argv) > 3 else 16

spacing = np.linspace(4.0, 40.0, ns)[:, None]            # ms between echoes
T2 = np.geomspace(20.0, 300.0, nt)[None, :]              # ms
T1, angle = 1200.0, 160.0                                # imperfect refocusing: stimulated echoes contribute
sigma2 = 1e-4                                            # noise variance for a unit signal at the excitation (SNR 100)

half = epg.E(spacing / 2, T1, T2, order1=["T2"])
seq = [epg.T(90, 90)] + [epg.S(1), half, epg.T(angle, 0), epg.S(1), half, epg.ADC] * necho

maps = {}
for unknowns, weights in ((["T2"], [1.0]), (["magnitude", "T2"], [0.0, 1.0])):
    jac = epg.simulate(seq, probe=epg.Jacobian(unknowns), out="device")        # [necho, ns, nt, len(unknowns)] in HBM
    maps[len(unknowns)] = stats.crlb(jac, W=weights, sigma2=sigma2, log=True)   # log10 of the variance bound of T2 [ms^2]

print(f"{necho} echoes, refocusing {angle:g} deg, sigma = {np.sqrt(sigma2):g}: best echo spacing per T2 (std bound of T2 in ms)")
print("    T2 [ms]   T2 alone            magnitude + T2")
for j in range(0, nt, max(nt // 8, 1)):
    cells = []
    for k in (1, 2):
        i = int(np.nanargmin(maps[k][:, j]))
        cells.append(f"{spacing[i, 0]:5.1f} ms ({10 ** (0.5 * maps[k][i, j]):.3f})")
    print(f"    {T2[0, j]:7.1f}   {cells[0]:18s}  {cells[1]}")
loss = 0.5 * (maps[2] - maps[1])
print(f"an unknown magnitude costs a factor {10 ** np.nanmin(loss):.2f} .. {10 ** np.nanmax(loss):.2f} in the std bound of T2 over the grid")

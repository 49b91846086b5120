"""A 3000-TR FISP-MRF train without max_nstate: the state matrix grows by one order per TR, as in the reference
(epgpy/shift.py:86,98), to 3001 orders -- beyond the capacity classes, so simulate() runs it on the tiled path
(DESIGN.md §4.5).

    python examples/unbounded_mrf.py
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import epgpy_amd as epg  # noqa: E402

NTR = 3000
T1 = np.linspace(300, 2500, 64)[:, None]
T2 = np.linspace(20, 300, 64)[None, :]
flips = 10 + 60 * np.abs(np.sin(np.arange(NTR) * np.pi / 500))

seq = [epg.T(180, 0), epg.E(20, T1, T2), epg.SPOILER]
for i, fa in enumerate(flips):
    seq += [epg.T(float(fa), 90.0 if i % 2 else 0.0), epg.E(2, T1, T2), epg.ADC, epg.E(8, T1, T2), epg.S(1)]

t0 = time.perf_counter()
sig = epg.simulate(seq)
print(f"{NTR} TRs x {T1.size * T2.size} voxels: signal {sig.shape}, {time.perf_counter() - t0:.2f} s, "
      f"|signal| at TR 1000 in [{abs(sig[1000]).min():.4f}, {abs(sig[1000]).max():.4f}]")

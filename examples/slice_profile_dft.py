"""Frequency profile of a sinc pulse, computed twice: with precession operators on a grid of off-resonance frequencies, and
with phase-state shifts read out in space by `epg.DFT` (the second half of the reference's examples/basics/pulse_profile.py).

    python examples/slice_profile_dft.py [--plot]

In the second form every sample of the pulse is followed by a shift S(1): the state matrix grows by one order per sample, and
a position x sees the dephasing k x per sample -- with kvalue = 2 pi f_max / (FOV / 2) * dt exactly the precession of the
frequency that belongs to x.  `DFT(positions)` sums the orders at every position on the device; nothing but the profile
([1, 301] values) comes back.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))   # run from a checkout
from epgpy_amd import epg  # noqa: E402

NPOINT, NLOBE, BW = 100, 5, 2.0            # samples, lobes, bandwidth (kHz)
DURATION = NLOBE / BW * 2                  # ms
T1, T2 = 1e3, 1e2
FOV = 1e-2                                 # m
offres = np.linspace(-3, 3, 301)           # kHz

wave = np.sinc(NLOBE * np.linspace(-1, 1, NPOINT))
pulse = epg.RFPulse(wave, DURATION, alpha=90)

# 1. off-resonance and relaxation inside the pulse, rewound by half the pulse's precession
with_p = epg.simulate([epg.modify(pulse, T1=T1, T2=T2, g=offres), epg.P(DURATION / 2, -offres), epg.ADC])[0]

# 2. one shift per sample, rewound by half the pulse's orders, read out at the positions of those frequencies
kvalue = 2 * np.pi * offres[-1] / (FOV / 2) * DURATION / NPOINT      # rad/m per order
relax, shift = epg.E(DURATION / NPOINT, T1, T2), epg.S(1)
positions = FOV * np.linspace(-0.5, 0.5, len(offres))
seq = [[t, relax, shift] for t in pulse.operators] + [epg.S(-NPOINT // 2), epg.DFT(positions)]
with_s = epg.simulate(seq, kvalue=kvalue)[0][0]

diff = float(np.max(np.abs(with_s - with_p)))
print("frequency (kHz)   |profile| (P)   |profile| (S + DFT)")
for i in range(0, len(offres), 25):
    print(f"{offres[i]:12.2f}   {abs(with_p[i]):12.6f}   {abs(with_s[i]):12.6f}")
print(f"largest difference between the two profiles: {diff:.2e}")
assert with_s.shape == with_p.shape == offres.shape and diff < 1e-9

if "--plot" in sys.argv:
    import matplotlib.pyplot as plt
    plt.plot(offres, np.abs(with_p), label="with P"), plt.plot(offres, np.abs(with_s), "--", label="with S and DFT")
    plt.xlabel("frequency (kHz)"), plt.ylabel("|F0|"), plt.legend(), plt.show()

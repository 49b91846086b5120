"""Multi-echo spin echo with realistic slice profiles: a 20-echo CPMG train whose excitation and refocusing pulses are
Hamming-windowed sincs under a slice-selection gradient, over (position across the slice x T2).

    python examples/slice_profile_mse.py [--plot]

The quantity of interest is the echo amplitude summed over the slice: imperfect refocusing at the slice edges mixes
stimulated echoes into the train, so the summed decay is NOT exp(-t / T2) -- the reason multi-echo T2 mapping fits EPG
models with slice profiles.  Each pulse is an `epg.RFPulse` (64 samples) made slice-selective by `epg.encode_phase`; the
device multiplies the samples of a pulse up once per voxel and applies the product as one operator per echo.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))   # run from a checkout
from epgpy_amd import epg  # noqa: E402

NECHO, ESP = 20, 10.0                      # echoes, echo spacing (ms)
T1, T2 = 1000.0, np.array([40.0, 80.0, 160.0])
GRADIENT, THICKNESS, NPOINT = 10.0, 5.0, 101      # mT/m, mm (nominal slice), positions over 3 slice thicknesses
DURATION = 2.0                             # ms per pulse

x = np.linspace(-3, 3, 64)
wave = np.sinc(x) * np.hamming(64)         # time-bandwidth product 6
bandwidth = 6 / DURATION                   # kHz
gradient = bandwidth / (epg.gamma_1H * 1e-6 * THICKNESS)      # mT/m for the nominal thickness
positions = epg.spatial_range(3 * THICKNESS, NPOINT)

exc = epg.encode_phase(epg.RFPulse(wave, DURATION, alpha=90, phi=90.0), gradient, positions, rewind=True)
rfc = epg.encode_phase(epg.RFPulse(wave, DURATION, alpha=180), gradient, positions)
wait = (ESP - DURATION) / 2
relax = epg.E(wait, T1, T2, duration=True)     # T2 along the first grid axis, positions along the second
crusher = epg.S(1)
train = [exc] + [relax, crusher, rfc, crusher, relax, epg.ADC] * NECHO

times, echoes = epg.simulate(train, adc_time=True)            # [NECHO, 3 T2, NPOINT]
over_slice = np.abs(echoes.sum(axis=-1)) / NPOINT
ideal = epg.simulate([epg.T(90, 90)] + [epg.E(ESP / 2, T1, T2), crusher, epg.T(180, 0), crusher, epg.E(ESP / 2, T1, T2), epg.ADC] * NECHO)

print("echo   t (ms)   " + "   ".join(f"T2 = {t:5.0f}: slice  hard" for t in T2))
for i in range(NECHO):
    print(f"{i + 1:4d}  {times[i]:7.2f}   " + "   ".join(f"          {over_slice[i, j]:7.4f} {abs(ideal[i, j]):6.4f}" for j in range(len(T2))))
# (a third of the positions lie inside the nominal slice; the hard-pulse train is the decay of a single isochromat)
assert echoes.shape == (NECHO, len(T2), NPOINT) and np.all(over_slice[0] < np.abs(ideal[0]))

if "--plot" in sys.argv:
    import matplotlib.pyplot as plt
    fig, (left, right) = plt.subplots(1, 2, figsize=(10, 4))
    for j, t2 in enumerate(T2):
        left.plot(times, over_slice[:, j], "o-", label=f"T2 = {t2:.0f} ms, summed over the slice")
        left.plot(times, np.abs(ideal[:, j]), "k:", lw=1)
    left.set_xlabel("time (ms)"), left.set_ylabel("echo amplitude"), left.legend()
    right.plot(positions, np.abs(echoes[0, 1]), label="echo 1"), right.plot(positions, np.abs(echoes[1, 1]), label="echo 2")
    right.set_xlabel("position (mm)"), right.set_ylabel("|F0|"), right.legend()
    plt.tight_layout(), plt.show()

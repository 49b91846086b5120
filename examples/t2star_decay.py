"""T2* decay after one excitation: the time accumulation operator C(tau, R2') adds tau * R2' to the fourth coordinate of the
state matrix, and F0 weighs every state by exp(-|t|) -- the free induction decay of a Lorentzian line, without isochromats.

    python examples/t2star_decay.py [necho]      # default 20

T(30, 90) tips 30 degrees; then 20 x [C(0.5 ms, 1 / 5 ms), ADC] with kgrid=0.1: the signal is 0.5 exp(-0.1 n).  The shift by a
float coordinate is the reference's shift-merge: which rows meet is planned on the host, the sums over the state run on the GPU.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))   # run from a checkout
from epgpy_amd import epg  # noqa: E402

necho = int(sys.argv[1]) if len(sys.argv) > 1 else 20
seq = [epg.T(30, 90)] + [epg.C(0.5, 1 / 5), epg.ADC] * necho
signal = np.asarray(epg.simulate(seq, kgrid=0.1)).reshape(-1)
expected = 0.5 * np.exp(-0.1 * np.arange(1, necho + 1))
for n, (got, want) in enumerate(zip(signal, expected), start=1):
    print(f"echo {n:3d}: |F0| = {abs(got):.12f}   0.5 exp(-0.1 n) = {want:.12f}")
print(f"max |difference| = {np.abs(signal - expected).max():.2e}")
assert np.abs(signal - expected).max() < 1e-12

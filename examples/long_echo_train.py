"""Long echo trains whose state matrix is never bounded -- the reference's default (shift.py:86,98: every S adds an order): a
CPMG train of N echoes ends with 2 N + 1 phase states.  The kernels walk such a train the way the state matrix grows (1, 2, 4 ...
orders per lane while it is short); derivative states travel with it in registers up to 1024 orders, and beyond that on the
tiled path when `mode="resident"` is written out (state and derivative windows in HBM): the last part feeds such a Jacobian,
left on the GPU, to stats.crlb.

    python examples/long_echo_train.py [n] [necho]        # n x n (T1, T2) grid, default 128 x 128, 250 echoes
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))   # run from a checkout
from epgpy_amd import epg  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 128
necho = int(sys.argv[2]) if len(sys.argv) > 2 else 250
T1 = np.linspace(200, 3000, n)[:, None]
T2 = np.linspace(40, 300, n)[None, :]
exc = epg.T(90, 90)
rfc = epg.T(150, 0, order1={"fa": {"alpha": 1.0}})          # d/d(refocusing angle), per degree
relax = epg.E(2.5, T1, T2, order1=["T2"])                     # d/dT2
shift = epg.S(1, duration=2.5)
seq = [exc] + [[shift, relax, rfc, shift, relax, epg.ADC]] * necho

enc, _, _ = epg.compile_sequence(seq)
print(f"{necho} echoes: {enc.peak + 1} phase states per voxel -> capacity {enc.capacity(resident=True)}")
epg.simulate(seq)
t0 = time.perf_counter()
signal = epg.simulate(seq)
dt = time.perf_counter() - t0
print(f"signal {signal.shape} in {1e3 * dt:.1f} ms = {signal.size / dt:.3e} echo*voxels/s")

# the same train with its Jacobian: [echo, *grid, (magnitude, dS/dT2, dS/dfa)]
t0 = time.perf_counter()
jac = epg.simulate(seq, probe=epg.Jacobian(["magnitude", "T2", "fa"]))
dt = time.perf_counter() - t0
c = n // 2
print(f"Jacobian {jac.shape} in {1e3 * dt:.1f} ms; centre voxel, last echo: |S| = {abs(jac[-1, c, c, 0]):.4f}, "
      f"dS/dT2 = {jac[-1, c, c, 1].real:+.3e} per ms, dS/dfa = {jac[-1, c, c, 2].real:+.3e} per degree")
h = 1e-3                                                        # (a central difference on T2 for the centre voxel)
up = epg.simulate([exc] + [[shift, epg.E(2.5, T1[c, 0], T2[0, c] + h), epg.T(150, 0), shift, epg.E(2.5, T1[c, 0], T2[0, c] + h), epg.ADC]] * necho)
dn = epg.simulate([exc] + [[shift, epg.E(2.5, T1[c, 0], T2[0, c] - h), epg.T(150, 0), shift, epg.E(2.5, T1[c, 0], T2[0, c] - h), epg.ADC]] * necho)
print(f"central difference: {((up[-1] - dn[-1]) / (2 * h)).real.item():+.3e}")

# beyond 1024 orders: the Jacobian of a 600-echo train (1201 phase states) on the tiled path, left in HBM for the Cramer-Rao bound
from epgpy_amd import stats  # noqa: E402

small = (slice(None, None, max(1, n // 32)),) * 2              # (a 32 x 32 corner of the grid keeps the example quick)
T1s, T2s = T1[small[0]], T2[:, small[1]]
relax_s = epg.E(2.5, T1s, T2s, order1=["T2"])
long = [exc] + [[shift, relax_s, rfc, shift, relax_s, epg.ADC]] * 600
try:
    epg.simulate(long, probe=epg.Jacobian(["magnitude", "T2"]))
except NotImplementedError as exc_info:
    print("mode='auto':", str(exc_info)[:90], "...")
t0 = time.perf_counter()
jac = epg.simulate(long, probe=epg.Jacobian(["magnitude", "T2"]), mode="resident", out="device")
bound = stats.crlb(jac, log=True)
dt = time.perf_counter() - t0
print(f"600 echoes, 1201 phase states: Jacobian {jac.shape} on the tiled path + CRLB map {bound.shape} in {1e3 * dt:.1f} ms; "
      f"log10 var(T2) from {bound.min():.2f} to {bound.max():.2f}")

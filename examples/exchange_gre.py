"""Gradient echoes of two-pool systems with exchange (EPG-X): Bloch-McConnell (BM) myelin-water exchange and a
magnetization-transfer (MT) bound pool, after Malik SJ, Teixeira RPAG, Hajnal JV, Magn Reson Med 2018; 80:767-779.

    python examples/exchange_gre.py

RF-spoiled SPGR (200 TR, five spoil increments) and balanced SSFP (500 TR over 101 off-resonance frequencies).  The bSSFP
signals after 500 TR are checked against the steady state of the linear two-pool model, solved directly.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))   # run from a checkout
from epgpy_amd import epg, exchange, magnettransfer  # noqa: E402

FA, TR = 10.0, 5.0                                # degrees, ms
# BM: a fast-relaxing myelin-water pool (20 %) exchanging with intra/extra-cellular water
bm = dict(T1=[1000.0, 500.0], T2=[100.0, 20.0], f=[0.8, 0.2], k=2e-3)
# MT: a free pool and a bound (semi-solid) pool with T2 of 12 us that the pulses saturate but do not rotate
mt = dict(T1=[779.0, 779.0], T2=[45.0, 12e-3], f=[1 - 0.117, 0.117], k=4.3e-3)
for model in (bm, mt):
    model["khi"] = exchange.exchange_matrix(model["k"], densities=model["f"])   # conserves the pool sizes

# saturation of the bound pool by a hard pulse of amplitude b1 (uT) lasting trf (ms), line value G (ms) at resonance
b1, G = 13.0, 15.1e-3
trf = np.deg2rad(FA) / (267.5221e-3 * b1)
W = magnettransfer.saturation_rate(trf, b1, G)
saturate = epg.R(rL=[0, trf * W])                 # bound pool's Z decays by exp(-trf W) per pulse

sum_pools = epg.Adc(reduce=0)                     # axis 0 holds the two pools
x_bm = epg.X(TR, bm["khi"], T1=bm["T1"], T2=bm["T2"])
x_mt = epg.X(TR, mt["khi"], T1=mt["T1"], T2=mt["T2"])

# ---- RF-spoiled SPGR: quadratic phase increments
increments = np.array([50.0, 84.0, 117.0, 150.0, 180.0])
pulses = [epg.T(FA, [n * (n + 1) / 2 * increments]) for n in range(200)]
spgr_bm = [[rf, sum_pools, x_bm, epg.S(1)] for rf in pulses]
spgr_mt = [[epg.T([FA, 0], rf.phi) @ saturate, sum_pools, x_mt, epg.S(1)] for rf in pulses]
s_bm = epg.simulate(spgr_bm, init=epg.StateMatrix(density=bm["f"]), max_nstate=100)
s_mt = epg.simulate(spgr_mt, init=epg.StateMatrix(density=mt["f"]), max_nstate=100)
print("SPGR after 200 TR, increments", increments)
print("  BM |signal|:", np.round(np.abs(s_bm[-1]), 5))
print("  MT |signal|:", np.round(np.abs(s_mt[-1]), 5))

# ---- bSSFP with alternating pulse phase
offres = np.linspace(-0.5, 0.5, 101) / TR        # kHz
x_bm_g = epg.X(TR, bm["khi"], T1=bm["T1"], T2=bm["T2"], g=[offres])
p0, p180 = epg.T(FA, 0), epg.T(FA, 180)
bssfp = [[p0, x_bm_g], [p180, x_bm_g]] * 250 + [[p0, sum_pools]]
s_bssfp = epg.simulate(bssfp, init=epg.StateMatrix(density=bm["f"]))[-1]


def bssfp_steady_state(model, df):
    """signal right after the pulse, in the steady state: per pool the vector (F+, F-, Z) obeys dm/dt = A m + c between
    pulses (relaxation, precession at df, exchange), so one TR maps m to E m + (E - 1) A^-1 c with E = exp(A TR); the
    pulse R follows, and the alternating phase is a 180 degree turn D about z: the steady state solves D m = R (E m + b)"""
    n = len(model["T1"])
    rates = []
    for t1, t2 in zip(model["T1"], model["T2"]):
        rates += [-1 / t2 + 2j * np.pi * df, -1 / t2 - 2j * np.pi * df, -1 / t1]
    A = np.diag(rates) - np.kron(model["khi"], np.eye(3))
    c = np.concatenate([[0, 0, f / t1] for f, t1 in zip(model["f"], model["T1"])])
    E = exchange.expm(A * TR)
    b = (E - np.eye(3 * n)) @ np.linalg.solve(A, c)
    R = np.kron(np.eye(n), p0.mat[0])
    D = np.kron(np.eye(n), np.diag([-1.0, -1.0, 1.0]))
    m = np.linalg.solve(D - R @ E, R @ b)
    return m[0::3].sum()                          # F+ at k = 0, summed over the pools


exact = np.array([bssfp_steady_state(bm, df) for df in offres])
err = float(np.max(np.abs(np.abs(s_bssfp) - np.abs(exact))))
print(f"bSSFP BM after 500 TR: max ||signal| - |steady state|| over {len(offres)} frequencies = {err:.2e}")
assert err < 2e-3, err
print("OK")

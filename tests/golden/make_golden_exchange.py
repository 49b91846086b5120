#!/usr/bin/env python3
"""Generate tests/golden/g17_exchange.npz from the reference: multi-compartment exchange (epgpy/exchange.py) and the
magnetization-transfer helpers (epgpy/magnettransfer.py).

Run ONLY in the build container, where the upstream reference (py-baudin/epgpy) is mounted read-only:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_exchange.py

As make_golden.py: the reference is imported as a black box and driven through its public API; only the resulting data
(inputs and expected outputs) are written.

Cases (G17):
  tables   X tables for a scalar rate and an N x N kinetic matrix, exchange_matrix(densities=), three compartments,
           axis=1, array tau / T1 / T2 / g, duration=True
  op       the scenarios of test/test_exchange.py::test_X_class as (input states, densities, output states), plus
           broadcast from one compartment, axis=1 and several tau
  mt       saturation_rate / absorption_rate (three line shapes)
  sim      simulate() signals: RF-spoiled SPGR (200 TR, max_nstate=100, five spoil phases) with Bloch-McConnell (BM) and
           MT pools, ADC and Adc(reduce=0); bSSFP BM over 101 off-resonances (500 TR); a three-compartment spin-echo train
           with g != 0 and S(1); a sequence whose compartment axis is axis 1
"""
import os
import sys

sys.dont_write_bytecode = True
REFERENCE = os.environ.get("EPGPY_REFERENCE", "/root/reference")
sys.path.insert(0, REFERENCE)

import numpy as np  # noqa: E402

if not hasattr(np, "asfarray"):      # (NumPy 2 removed it; the reference's spline helper still calls it)
    np.asfarray = lambda a: np.asarray(a, dtype=np.float64)

import epgpy as epg  # noqa: E402  (the reference)
from epgpy import exchange, magnettransfer, operators, functions, statematrix  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = {}


def put(name, value):
    OUT[name] = np.asarray(value)


# ------------------------------------------------------------------------------------------------------------ tables
put("tab_scalar", exchange.X(5, 0.01, T1=[1000, 500], T2=[100, 20]).mat)
kmat3 = np.array([[0.03, -0.01, -0.02], [-0.02, 0.03, -0.01], [-0.01, -0.02, 0.03]])
put("kmat3", kmat3)
put("tab_n3", exchange.X(7, kmat3, T1=[800, 1000, 300], T2=[60, 80, 15], g=[0, 0.01, -0.02]).mat)
put("exm_dens", exchange.exchange_matrix(2e-3, densities=[0.8, 0.2]))
put("exm_k", exchange.exchange_matrix([1e-3, 2e-3, 5e-3], axis=1, ncomp=2))
put("exm_n3", exchange.exchange_matrix(0.02, ncomp=3))
khi_ax1 = exchange.exchange_matrix([0.01, 0.02, 0.05], axis=1)          # (3, 2, 2): compartments on axis 1
put("khi_ax1", khi_ax1)
x_ax1 = exchange.X(5, khi_ax1, axis=1, T1=[[900, 400]], T2=[[70, 25]])
put("tab_ax1", x_ax1.mat)
put("tab_ax1_axis", x_ax1.axis)
taus, T1s, T2s, gs = np.array([[2.0, 5.0, 10.0]]), [1000, 500], [100, 20], [[0.0], [0.05]]
x_arr = exchange.X(taus, 0.01, T1=T1s, T2=T2s, g=gs)
put("tab_arr", x_arr.mat)
put("tab_arr_shape", x_arr.shape)
put("tab_arr_in", np.asarray(taus))
x_dur = exchange.X(4.5, 0.01, duration=True)
put("dur_true", x_dur.duration)
rng = np.random.default_rng(17)
A = rng.uniform(-1, 1, (3, 3)) + 1j * rng.uniform(-1, 1, (3, 3))
put("expm_in", A)
put("expm_out", exchange.expm(A))
H = A + A.T.conj()
put("expm_herm_in", H)
put("expm_herm_out", exchange.expm(H))


# ------------------------------------------------------------------------------------------------------------ op(sm)
def op_case(name, op, sm):
    put(f"op_{name}_in", sm.states)
    put(f"op_{name}_dens", sm.density)
    put(f"op_{name}_out", op(sm).states)


sm0 = statematrix.StateMatrix([1, 1, 0])
sm0j = statematrix.StateMatrix([[[1, 1, 0]], [[1j, -1j, 0]]])
sm0x = statematrix.StateMatrix([[[1, 1, 0]], [[3, 3, 0]]], density=[1, 3])
op_case("noexchange", exchange.X(10, 0), sm0)
op_case("same", exchange.X(10, 0.1), sm0)
op_case("mixed", exchange.X(10, 1), sm0j)
op_case("relax", exchange.X(10, 0, T2=[np.inf, 1e-8]), sm0)
op_case("fastrelax", exchange.X(10, 10, T2=[np.inf, 1e-8]), sm0)
op_case("mean", exchange.X(10, 1e10, T2=[30, 40]), sm0)
op_case("recovery", exchange.X(10, 0, T1=1e-10, T2=1e-10), sm0x)
op_case("densities", exchange.X(10, [[3e10, -1e10], [-3e10, 1e10]]), sm0x)
states = rng.normal(size=(2, 5, 3)) + 1j * rng.normal(size=(2, 5, 3))
states[..., 0] = states[..., ::-1, 1].conj()      # F+ / F- symmetry of a state matrix with two phase orders
states[..., 2, 2] = states[..., 2, 2].real
states[..., 2] = 0.5 * (states[..., 2] + states[..., ::-1, 2].conj())
sm_r = statematrix.StateMatrix(states, density=[0.8, 0.2])
op_case("unequal", exchange.X(5, exchange.exchange_matrix(0.05, densities=[0.8, 0.2]), T1=[900, 300], T2=[80, 20],
                               g=[0, 0.02]), sm_r)
sm_ax1 = statematrix.StateMatrix(np.broadcast_to(states[0], (3, 2, 5, 3)), density=[[0.5, 0.5]] * 3)
op_case("axis1", x_ax1, sm_ax1)
op_case("taus", x_arr, statematrix.StateMatrix(states[0], shape=None))
kbad = exchange.exchange_matrix(0.05)                # conserves equal densities only
put("op_bad_khi", kbad)
put("op_bad_dens", [0.8, 0.2])

# ------------------------------------------------------------------------------------------------------------ MT
put("mt_sat_hard", magnettransfer.saturation_rate(0.5, 13.0, 15.1e-3))
wave = np.sin(np.linspace(0, np.pi, 33)) * 10.0
put("mt_sat_wave_in", wave)
put("mt_sat_wave", magnettransfer.saturation_rate(2.0, wave, 15.1e-3))
offres = np.array([-8.0, -3.0, -1.0, 0.0, 0.3, 0.9, 1.0, 2.5, 5.0, 12.0])
put("mt_offres", offres)
for shape in ("gaussian", "lorentzian", "super-lorentzian"):
    put(f"mt_abs_{shape}", magnettransfer.absorption_rate(12e-3, shape, offres))

# ------------------------------------------------------------------------------------------------------------ simulate
FA, TR, NRF = 10, 5.0, 200
PH = np.array([50.0, 84.0, 117.0, 150.0, 180.0])
model_bm = dict(T1=[1000, 500], T2=[100, 20], f=[0.8, 0.2], khi=2e-3)
model_mt = dict(T1=[779, 779], T2=[45, 12e-3], f=[1 - 0.117, 0.117], khi=4.3e-3)
k_bm = exchange.exchange_matrix(model_bm["khi"], densities=model_bm["f"])
k_mt = exchange.exchange_matrix(model_mt["khi"], densities=model_mt["f"])
b1, G = 13.0, 15.1e-3
gamma = 267.5221e-3
trf = (np.pi / 180 * FA) / (gamma * b1)
W = magnettransfer.saturation_rate(trf, b1, G)
put("sim_params", [FA, TR, NRF, b1, G, trf, W])
put("sim_ph", PH)
put("sim_k_bm", k_bm)
put("sim_k_mt", k_mt)

adc_sum = operators.Adc(reduce=0)
exg = operators.X(TR, k_bm, T1=model_bm["T1"], T2=model_bm["T2"])
mt = operators.X(TR, k_mt, T1=model_mt["T1"], T2=model_mt["T2"])
sat = operators.R(rL=[0, trf * W])
rfs = [operators.T(FA, [i * (i + 1) / 2 * PH]) for i in range(NRF)]
shift = operators.S(1)
seq_bm = [[rf, operators.ADC, exg, shift] for rf in rfs]
seq_bm_sum = [[rf, adc_sum, exg, shift] for rf in rfs]
seq_mt_sum = [[operators.T([FA, 0], rf.phi) @ sat, adc_sum, mt, shift] for rf in rfs]
put("sim_spgr_bm", functions.simulate(seq_bm, max_nstate=100, init=statematrix.StateMatrix(density=model_bm["f"])))
put("sim_spgr_bm_sum", functions.simulate(seq_bm_sum, max_nstate=100, init=statematrix.StateMatrix(density=model_bm["f"])))
put("sim_spgr_mt_sum", functions.simulate(seq_mt_sum, max_nstate=100, init=statematrix.StateMatrix(density=model_mt["f"])))

NSSFP, NOFF = 500, 101
offres = 1 / TR * np.linspace(-0.5, 0.5, NOFF)
exg_g = operators.X(TR, k_bm, T1=model_bm["T1"], T2=model_bm["T2"], g=[offres])
rf1, rf2 = operators.T(FA, 0), operators.T(FA, 180)
seq_bssfp = [[rf1, exg_g], [rf2, exg_g]] * (NSSFP // 2) + [[rf1, adc_sum]]
put("sim_bssfp_bm", functions.simulate(seq_bssfp, init=statematrix.StateMatrix(density=model_bm["f"])))

# three compartments, spin echoes with chemical shift and S(1)
x3 = operators.X(5.0, kmat3, T1=[800, 1000, 300], T2=[60, 80, 15], g=[0, 0.01, -0.02])
seq_se = [operators.T(90, 90)] + [[shift, x3, operators.T(150, 0), shift, x3, operators.ADC]] * 12
put("sim_se3", functions.simulate(seq_se, init=statematrix.StateMatrix(density=[1.0, 1.0, 1.0])))

# compartments on axis 1 (axis 0: three flip angles)
x_a1 = operators.X(TR, khi_ax1, axis=1, T1=[[900, 400]], T2=[[70, 25]])
seq_a1 = [operators.T([[20.0], [40.0], [60.0]], 90)] + [[shift, x_a1, operators.T(120, 0), shift, x_a1, operators.ADC]] * 10
put("sim_axis1", functions.simulate(seq_a1, init=statematrix.StateMatrix(density=[[0.5, 0.5]] * 3)))

path = os.path.join(HERE, "g17_exchange.npz")
np.savez_compressed(path, **OUT)
print("wrote", path, os.path.getsize(path), "bytes")

"""Sequence design with second derivatives: a few gradient steps on the refocusing angles of a short multi-spin-echo train,
minimising the Cramer-Rao bound of T2 (magnitude unknown as well) averaged over a range of T2.

The cost needs the Jacobian of the signal w.r.t. (magnitude, T2) and its derivative w.r.t. every angle -- a Hessian over
(tissue parameter x design variable) pairs.  `simulate(..., mode="resident")` computes each pair in ONE launch of the fused
second-order kernel (state, both first-order states and the second-order state of a voxel in registers) instead of hundreds
of launches operator by operator.  Both calls leave their records in HBM (`out="device"`; a Jacobian and a Hessian probe do not
share a device call), and `stats.crlb_grad` computes cost and gradient there: only the two maps cross PCIe.

    python examples/optim_mse_crlb.py [necho] [n_T2] [steps]      # defaults 8, 32, 6
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))   # run from a checkout
from epgpy_amd import epg, stats  # noqa: E402

necho = int(sys.argv[1]) if len(sys.argv) > 1 else 8
nt = int(sys.argv[2]) if len(sys.argv) > 2 else 32
steps = int(sys.argv[3]) if len(sys.argv) > 3 else 6

T1, spacing, sigma2 = 1200.0, 10.0, 1e-4
T2 = np.geomspace(30.0, 200.0, nt)
angles = np.full(necho, 140.0)
names = [f"a{i}" for i in range(necho)]


def cost_and_gradient(angles):
    pairs = [("T2", name) for name in names]
    half = epg.E(spacing / 2, T1, T2, order1=["T2"], order2=pairs)
    pulses = [epg.T(float(a), 0, order1={name: "alpha"}, order2=[("T2", name)]) for a, name in zip(angles, names)]
    seq = [epg.T(90, 90)]
    for rf in pulses:
        seq += [epg.S(1), half, rf, epg.S(1), half, epg.ADC]
    jac = epg.simulate(seq, probe=epg.Jacobian(["magnitude", "T2"]), out="device")                               # [necho, n_T2, 2]
    hes = epg.simulate(seq, probe=epg.Hessian(["magnitude", "T2"], names), mode="resident", out="device")       # [necho, n_T2, 2, necho]: d(dS/dp)/d(angle)
    cost, grad = stats.crlb_grad(jac, hes, W=[0.0, 1.0], sigma2=sigma2, log=True)
    return float(np.mean(cost)), np.mean(grad, axis=0)


rate = 400.0                                 # degrees^2 per unit of log10 variance
for step in range(steps):
    cost, grad = cost_and_gradient(angles)
    print(f"step {step}: mean log10 variance bound of T2 = {cost:.5f}   angles = {np.round(angles, 1).tolist()}")
    angles = np.clip(angles - rate * grad, 60.0, 180.0)
cost, _ = cost_and_gradient(angles)
print(f"final : mean log10 variance bound of T2 = {cost:.5f}   angles = {np.round(angles, 1).tolist()}")

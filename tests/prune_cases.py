"""The sequences of tests/golden/g23_prune.npz: per-voxel float shifts ('shift-prune').  `build(epg, name)` returns
(operators, options) for any module with the reference's public interface; the generator runs them through the reference, the
tests through the package.  In every case each shift that follows a per-voxel one is itself per voxel (the package's
broadcast of a scalar shift onto per-voxel coordinates deviates from the reference on purpose and stays out of the cases)."""
import numpy as np

CASES = ("s_recombine", "g_trim", "gre_t2prime", "g_c_mixed")


def build(epg, name):
    if name == "s_recombine":
        # kdim 1; voxel 1 does not move, voxel 2 is never excited (alpha = 0: its shifted rows are empty and leave with the
        # prune while the others keep theirs); S(-0.5 k) after S(k) lets the states recombine
        k = np.array([1.5, 0.0, 0.9, 2.3, -1.2])
        alpha = np.array([65.0, 50.0, 0.0, 80.0, 55.0])
        ops = []
        for i in range(3):
            ops += [epg.T(alpha, 90.0 + 20.0 * i), epg.E(3.0, 900.0, 60.0), epg.S(k[:, None]), epg.ADC,
                    epg.T(alpha, 30.0), epg.S(-0.5 * k[:, None]), epg.ADC]
        return ops, dict(kgrid=0.25)
    if name == "g_trim":
        # kdim 3: a gradient per voxel, at most 4 positive rows per voxel
        grad = np.array([[1.0, 0.0, 0.0], [0.6, -0.8, 0.0], [0.3, 0.5, -0.9], [0.0, 0.0, 1.2]])
        ops = []
        for i in range(4):
            ops += [epg.T(np.array([40.0, 55.0, 70.0, 85.0]) + 5.0 * i, 117.0 * i * i), epg.E(2.0 + 0.7 * i, 800.0, 70.0), epg.ADC, epg.G(1.0 + 0.3 * i, grad)]
        return ops, dict(kgrid=40.0, max_nstate=4)
    if name == "gre_t2prime":
        # kdim 4: a GRE train over a (T2', T2) grid; ADC weighs the rows with exp(-|t|)
        T2, R2 = np.array([40.0, 80.0, 120.0, 200.0]), np.array([0.02, 0.05, 0.11])
        ops = []
        for i in range(6):
            ops += [epg.T(np.array([[20.0], [25.0], [30.0]]), 50.0 * i), epg.E(2.0, 1000.0, T2[None, :]), epg.C(2.0, R2[:, None]), epg.ADC]
        return ops, dict(kgrid=0.011)
    if name == "g_c_mixed":
        # kdim 4: a gradient along the first grid axis, T2' along the second
        grad = 1e-3 * np.array([[0.5, 0.0, 0.0], [0.0, 0.7, 0.0], [0.4, 0.0, -0.6]])[:, None, :]
        R2 = np.array([0.034, 0.088])[None, :]
        ops = []
        for i in range(4):
            ops += [epg.T(np.array([[30.0], [35.0], [40.0]]), 90.0 * i), epg.E(1.5, 1000.0, 90.0), epg.G(1.0, grad), epg.C(1.5, R2), epg.ADC]
        return ops, dict(kgrid=0.02)
    raise KeyError(name)

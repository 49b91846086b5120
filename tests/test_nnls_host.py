"""CPU: `match.nnls_host`, the NumPy statement of the method of `match.nnls`, against `scipy.optimize.nnls` on the stacked real
system, both judged by the extended-precision yardstick of tests/nnls_cases.py (J from the raw dictionary, no Gram matrix); what
the GPU test relies on (status 0 on every voxel of every regular case, a passive set that reaches all A atoms, atoms that leave);
every status and degenerate rule; `fraction`, `gmean`, `unravel`; the boundary (header, binding, ABI 11); and the refusals of
`Components` and `nnls` that need no device."""
import os
import re

import numpy as np
import pytest

from epgpy_amd import _build, _lib, match
from tests import nnls_cases as nc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = nc.cases()
_HOST = {}


def host(name):
    if name not in _HOST:
        c = CASES[name]
        _HOST[name] = match.nnls_host(c["D"], c["S"], c["axis"], reg=c["reg"])
    return _HOST[name]


@pytest.mark.parametrize("name", sorted(CASES))
def test_host_against_scipy(name):
    """J(nnls_host) <= J(scipy) (1 + MARGIN) and the other way round, in the group nnls_host chose; where reg >= 1e-4 the weights
    agree within the bound from cond(H + mu I); the chosen group has the smallest J of scipy's solutions too"""
    c = CASES[name]
    y = nc.Yardstick(c["D"], c["S"], c["axis"], c["reg"])
    ref = nc.scipy_reference(c["D"], c["S"], c["axis"], c["reg"])
    res = host(name)
    A, nmeas = y.A, c["S"].shape[1]
    assert res.weights.shape == (A, nmeas) and res.group.dtype == np.int64 and res.status.dtype == np.int32
    assert (res.status == 0).all(), "every voxel of a regular case is solved"
    assert (res.weights >= 0).all()
    cond = nc.cond_ridge(c["D"], c["axis"], c["reg"])
    over, under = 0.0, 0.0
    for m in range(nmeas):
        g = int(res.group[m])
        Jh, Js = y.J(m, g, res.weights[:, m]), y.J(m, g, ref[g, :, m])
        over, under = max(over, float(Jh / Js - 1)), max(under, float(Js / Jh - 1))
        assert Jh <= Js * (1 + nc.MARGIN) and Js <= Jh * (1 + nc.MARGIN), (name, m, float(Jh), float(Js))
        every = [y.J(m, k, ref[k, :, m]) for k in range(y.G)]
        assert Js <= min(every) * (1 + nc.MARGIN), (name, m, "not the best group")
        assert abs(res.residual[m] - float(y.residual(m, g, res.weights[:, m]))) <= nc.residual_tol(y.nrec, y.A, y.energy(m))
        if c["reg"] >= 1e-4:
            assert np.max(np.abs(res.weights[:, m] - ref[g, :, m])) <= nc.weight_tol(cond[g], ref[g, :, m]), (name, m)
    print(name, "J over scipy:", over, "scipy over J:", under, "cond:", cond.max())


def test_cases_cover_what_the_kernel_turns_on():
    shapes = [(nc.split(c["D"], c["axis"]).shape, c["S"].shape[1]) for c in CASES.values()]
    assert {s[0][1] for s in shapes} >= {1, 3, 33, 40, 64}
    assert {s[0][0] for s in shapes} >= {1, 8, 33}
    assert {s[0][2] for s in shapes} >= {1, 3}
    assert {s[1] for s in shapes} >= {1, 65, 130}
    assert [CASES[k]["axis"] for k in ("axis_first", "axis_middle", "axis_last")] == [0, 1, 2]
    assert all(CASES[k]["D"].ndim == 4 for k in ("axis_first", "axis_middle", "axis_last"))
    for name in ("full_a64_r80_g1_m9", "full_a40_r48_g3_m1"):
        assert CASES[name]["reg"] == 1e-2
        assert ((host(name).weights > 0).sum(axis=0) == host(name).weights.shape[0]).any(), "the passive set reaches all A atoms"
    assert host("a33_r33_g3_m130").left.sum() > 100 and host("a64_r33_g3_m65").left.sum() > 50, "atoms leave the passive set"
    assert any(np.abs(c["D"].imag).max() == 0 for c in CASES.values()) and any(np.abs(c["D"].imag).max() > 0 for c in CASES.values())
    assert any(c["reg"] == 0.0 for c in CASES.values())


def test_degenerate_rules():
    c = nc.special()
    D, S = c["D"], c["S"]
    res = match.nnls_host(D, S, 0, reg=c["reg"])
    assert res.groups == (4,) and res.weights.shape == (6, 7)
    # the all-zero signal: weights 0, status 0, residual 0, group 0
    assert (res.weights[:, 0] == 0).all() and res.status[0] == 0 and res.residual[0] == 0 and res.group[0] == 0
    # group 1: the NaN atom and the all-zero atom carry 0 and the rest is found
    assert (res.group[1:4] == 1).all() and (res.weights[[2, 4], 1:4] == 0).all() and (res.weights[[0, 1, 3, 5], 1:4] > 0).any()
    assert (res.status == 0).all() and np.isfinite(res.weights).all()
    # groups 0 and 3 are the same atoms: the lower index
    assert (res.group[4:] == 0).all()
    fixed = match.nnls_host(D, S, 0, reg=c["reg"], group=np.array([3, 1, 1, 0, 3, 0, 2]))
    assert fixed.group.tolist() == [3, 1, 1, 0, 3, 0, 2]
    assert fixed.weights[:, [1, 2, 5]].tobytes() == res.weights[:, [1, 2, 5]].tobytes()
    assert fixed.weights[:, 4].tobytes() == res.weights[:, 4].tobytes()            # group 3 = group 0, to the bit
    # a group whose atoms are all invalid: weights 0, the whole signal is residual
    assert (fixed.weights[:, 6] == 0).all() and fixed.status[6] == 0
    assert abs(fixed.residual[6] - np.linalg.norm(S[:, 6])) <= 1e-12 * np.linalg.norm(S[:, 6])
    out = match.nnls_host(D, S, 0, reg=c["reg"], group=np.array([-1, 4, 0, 0, 0, 0, 0]))
    assert out.group[:2].tolist() == [-1, -1] and np.isnan(out.weights[:, :2]).all() and np.isnan(out.residual[:2]).all()
    assert (out.status[:2] == 2).all() and (out.status[2:] == 0).all()
    # a signal that is not finite: every group is skipped
    bad = S.copy()
    bad[3, 2] = np.nan
    bad[0, 5] = np.inf
    out = match.nnls_host(D, bad, 0, reg=c["reg"])
    assert out.group[[2, 5]].tolist() == [-1, -1] and (out.status[[2, 5]] == 2).all() and np.isnan(out.weights[:, [2, 5]]).all()
    assert out.weights[:, [1, 3, 4, 6]].tobytes() == res.weights[:, [1, 3, 4, 6]].tobytes()


def test_status_rules_of_one_task():
    ok = np.ones(2, dtype=bool)
    # a pivot <= 0: atom 0 enters, then atom 1 with pivot 1 - 4
    x, J, Jd, st, ns, nl = match._nnls_task(np.array([[1.0, -2.0], [-2.0, 1.0]]), ok, 0.0, np.array([1.0, 0.5]), 1.0, 1e-10)
    assert st == 2 and np.isnan(x).all() and np.isnan(J)
    # the cap: the weights are the last feasible iterate
    c = CASES["a33_r33_g3_m130"]
    Dg = nc.split(c["D"], 0)[:, :, 0]
    H = (np.conj(Dg).T @ Dg).real
    f = (np.conj(Dg).T @ c["S"][:, 0]).real
    E = float((np.abs(c["S"][:, 0]) ** 2).sum())
    mu = 1e-8 * np.trace(H) / 33
    full = match._nnls_task(H, np.ones(33, dtype=bool), mu, f, E, 1e-10)
    assert full[3] == 0 and 4 < full[4] <= 99
    cut = match._nnls_task(H, np.ones(33, dtype=bool), mu, f, E, 1e-10, cap=4)
    assert cut[3] == 1 and cut[4] == 4 and np.isfinite(cut[0]).all() and (cut[0] >= 0).all() and cut[1] > full[1]
    assert match._nnls_task(H, np.ones(33, dtype=bool), mu, f, E, 1e-10, cap=99)[0].tobytes() == full[0].tobytes()     # 3 A is the default
    # tol is a condition: with tol = 1 no atom can enter (Cauchy-Schwarz)
    none = match._nnls_task(H, np.ones(33, dtype=bool), mu, f, E, 1.0)
    assert (none[0] == 0).all() and none[3] == 0 and none[1] == E


def test_fraction_gmean_unravel():
    w = np.zeros((4, 2, 3))
    w[:, 0, 0] = [1.0, 1.0, 2.0, 0.0]
    w[:, 1, 2] = [0.0, 0.0, 0.0, 5.0]
    w[:, 1, 1] = np.nan
    grp = np.array([[0, 5, -1], [3, -1, 2]])
    res = match.NnlsResult(w, grp, None, None, (2, 3))
    vals = [10.0, 20.0, 40.0, 80.0]
    fr = res.fraction(10.0, 40.0, vals)
    assert fr.shape == (2, 3) and fr[0, 0] == 0.5 and fr[1, 2] == 0.0 and np.isnan(fr[0, 1]) and np.isnan(fr[1, 1])
    assert res.fraction(0.0, 100.0, vals)[0, 0] == 1.0
    gm = res.gmean(vals)
    assert abs(gm[0, 0] - np.exp((np.log(10) + np.log(20) + 2 * np.log(40)) / 4)) < 1e-12 and abs(gm[1, 2] - 80.0) < 1e-12
    assert np.isnan(gm[0, 1])
    a, b = res.unravel()
    assert a.tolist() == [[0, 1, -1], [1, -1, 0]] and b.tolist() == [[0, 2, -1], [0, -1, 2]]
    assert match.NnlsResult(w[:, 0, 0], np.array(0), None, None, ()).unravel() == ()
    with pytest.raises(ValueError, match="values"):
        res.fraction(0, 1, [1.0, 2.0])


def test_boundary_agrees():
    """include/epgx.h, _lib.py, _build.py and the built library: the new entry points within ABI 11"""
    header = open(os.path.join(ROOT, "include", "epgx.h")).read()
    assert "#define EPGX_ABI_VERSION 11" in header and _lib.ABI_VERSION == 11
    for entry, nargs in (("epgx_signal_component_gram", 10), ("epgx_signal_nnls", 20)):
        proto = re.search(r"int %s\(([^)]*)\)" % entry, header).group(1)
        assert len(proto.split(",")) == len(_lib.SYMBOLS[entry][1]) == nargs
    lib = _lib.load()
    assert lib.epgx_abi_version() == 11 and hasattr(lib, "epgx_signal_nnls") and hasattr(lib, "epgx_signal_component_gram")
    assert any(src == "epgx_nnls.hip" for _, src, _ in _build.UNITS)
    assert match.MAX_COMPONENTS == _lib.NNLS_MAX_A == 64
    for line in ("H_g[a,b] = Re sum_t conj(D[t,a,g]) D[t,b,g]", "f[a]     = Re sum_t conj(D[t,a,g]) S[t,m]",
                 "mu_g     = reg * (trace(H_g over the valid atoms) / (number of valid atoms))"):
        assert line in header and line in match.__doc__, line


def test_refusals_without_a_device():
    from epgpy_amd import functions
    D = np.zeros((4, 65, 3), dtype=np.complex128)
    with pytest.raises(NotImplementedError, match="1 .. 64"):
        match.Components(D, 0)
    for bad in (2, -3, 0.5):
        with pytest.raises(ValueError, match="axis"):
            match.Components(D, bad)
    with pytest.raises(ValueError, match="grid axis"):
        match.Components(np.zeros(4), 0)
    with pytest.raises(NotImplementedError, match="ShardedDeviceSignal"):
        match.Components(object.__new__(functions.ShardedDeviceSignal), 0)
    with pytest.raises(NotImplementedError, match="DeviceHessian"):
        match.Components(object.__new__(functions.DeviceHessian), 0)
    with pytest.raises(ValueError, match="Components"):
        match.nnls(D, np.zeros((4, 2)))
    c = CASES["a3_r8_g3_m65"]
    for kw in (dict(reg=-1e-3), dict(reg=np.nan), dict(reg=np.inf), dict(tol=-1.0), dict(tol=np.nan)):
        with pytest.raises(ValueError, match="reg|tol"):
            match.nnls_host(c["D"], c["S"], 0, **kw)
    with pytest.raises(ValueError, match="group"):
        match.nnls_host(c["D"], c["S"], 0, group=np.zeros(64, dtype=np.int64))
    with pytest.raises(ValueError, match="integer"):
        match.nnls_host(c["D"], c["S"], 0, group=np.zeros(65))
    with pytest.raises(ValueError, match="nnls_host"):
        match.nnls_host(c["D"], c["S"][:7], 0)
    assert match.nnls_host(c["D"], c["S"], -2).weights.tobytes() == host("a3_r8_g3_m65").weights.tobytes()

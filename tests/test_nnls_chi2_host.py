"""CPU: the chi^2-driven ridge as `epgpy_amd.match.nnls_host(..., chi2=)` defines it (the method of the `match` module docstring),
against the extended-precision quantities and the scipy + brentq reference of tests/nnls_chi2_cases.py.  It shows that the
reference stays inside the conditions the GPU tests set: every voxel of every regular case reaches status 0 by `nnls_host`, and
`scipy.optimize.nnls` inside `scipy.optimize.brentq` reaches the same condition on its own.  The evaluation counts printed here
are the ones DESIGN 4.17 takes the expansion factor and the cap from."""
import numpy as np
import pytest

from tests import nnls_cases as nc
from tests import nnls_chi2_cases as cc

CASES = cc.cases()
_HOST = {}


def host(name):
    from epgpy_amd import match
    if name not in _HOST:
        c = CASES[name]
        _HOST[name] = (match.nnls_host(c["D"], c["S"], c["axis"], reg=c["reg"]),
                       match.nnls_host(c["D"], c["S"], c["axis"], reg=c["reg"], chi2=c["chi2"]))
    return _HOST[name]


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_voxel_reaches_the_condition(name):
    """status 0 everywhere; the chi^2 condition, the optimality at the returned ridge and the structure in extended precision;
    the reference (scipy inside brentq) reaches the condition on its own, on a subset of the voxels"""
    c = CASES[name]
    plain, res = host(name)
    y = nc.Yardstick(c["D"], c["S"], c["axis"], c["reg"])
    nmeas, chi2 = c["S"].shape[1], c["chi2"]
    assert (plain.status == 0).all() and (res.status == 0).all()
    assert res.mu.dtype == np.float64 and res.chi2.dtype == np.float64 and res.evals.dtype == np.int32
    assert res.group.tobytes() == plain.group.tobytes()
    assert (res.weights >= 0).all() and (res.evals <= cc.EVALS).all()
    print(name, "evals: max", res.evals.max(), "mean", res.evals.mean())
    for m in range(nmeas):
        g = int(res.group[m])
        E = y.energy(m)
        Jd0 = cc.misfit(y, m, g, plain.weights[:, m])
        Jd = cc.misfit(y, m, g, res.weights[:, m])
        slack = 2 * cc.gram_rounding(y.nrec, y.A, E) / float(Jd0)
        assert abs(float(Jd / Jd0) - chi2) / chi2 <= cc.RTOL + slack, (name, m)
        assert abs(res.chi2[m] - float(Jd / Jd0)) <= chi2 * slack
        assert abs(res.residual[m] - float(np.sqrt(Jd))) <= nc.residual_tol(y.nrec, y.A, E)
        assert res.mu[m] >= float(y.mu[g]) * (1 - 1e-15)
        assert (res.weights[:, m] ** 2).sum() <= (plain.weights[:, m] ** 2).sum() * (1 + nc.MARGIN)
        sp = cc.scipy_at(y, m, g, res.mu[m])
        Jh, Js = cc.objective(y, m, g, res.weights[:, m], res.mu[m]), cc.objective(y, m, g, sp, res.mu[m])
        assert Jh <= Js * (1 + nc.MARGIN) and Js <= Jh * (1 + nc.MARGIN), (name, m, float(Jh), float(Js))
    for m in sorted({0, nmeas // 2, nmeas - 1}):
        g = int(res.group[m])
        mu, x, r = cc.scipy_brentq(y, m, g, chi2)
        assert abs(r) <= cc.RTOL and mu >= float(y.mu[g])
        # both ridges lie where the misfit is within rtol of the target, and the misfit grows with the ridge
        lo, hi = sorted([mu, res.mu[m]])
        assert cc.misfit(y, m, g, cc.scipy_at(y, m, g, lo)) <= cc.misfit(y, m, g, cc.scipy_at(y, m, g, hi)) * (1 + nc.MARGIN)
    if c["decay"] and y.A > 1:      # (one atom: the passive set cannot grow)
        assert ((res.weights > 0).sum(axis=0) > (plain.weights > 0).sum(axis=0)).any(), "a search that never moves"


def test_evaluation_counts():
    """the largest and the mean number of fits over the regular cases stay where DESIGN 4.17 records them: far below the cap"""
    evals = np.concatenate([host(name)[1].evals.reshape(-1) for name in sorted(CASES)])
    print("evals over the cases: max", evals.max(), "mean", evals.mean(), "histogram", np.bincount(evals).tolist())
    assert evals.max() <= cc.EVALS // 2


def test_chi2_none_changes_nothing():
    from epgpy_amd import match
    c = CASES["axis_middle"]
    a = match.nnls_host(c["D"], c["S"], c["axis"], reg=c["reg"])
    b = match.nnls_host(c["D"], c["S"], c["axis"], reg=c["reg"], chi2=None)
    for f in ("weights", "group", "residual", "status", "solves", "left"):
        assert getattr(a, f).tobytes() == getattr(b, f).tobytes()
    assert a.mu is None and a.chi2 is None and a.evals is None


def test_statuses_3_and_4():
    """status 4: a noise-free atom and an all-zero signal; status 3: a signal orthogonal to every atom, a weak fit against a large
    chi2, and the cap of evaluations (lowered through the private argument, as the cap of 3 A solves is held)"""
    from epgpy_amd import match
    e = cc.edge()
    plain = match.nnls_host(e["D"], e["S"], 0, reg=e["reg"])
    res = match.nnls_host(e["D"], e["S"], 0, reg=e["reg"], chi2=e["chi2"])
    assert res.status.tolist() == [4, 3, 3, 0, 4]
    untouched = [0, 1, 2, 4]
    assert res.weights[:, untouched].tobytes() == plain.weights[:, untouched].tobytes()
    assert res.residual[untouched].tobytes() == plain.residual[untouched].tobytes()
    mu0 = e["reg"] * np.mean(np.sum(np.abs(e["D"]) ** 2, axis=0))
    assert np.allclose(res.mu[untouched], mu0, rtol=1e-14, atol=0) and (res.chi2[untouched] == 1).all() and (res.evals[untouched] == 0).all()
    assert res.evals[3] > 0 and abs(res.chi2[3] / e["chi2"] - 1) <= cc.RTOL and res.mu[3] > mu0
    full = int(res.evals[3])
    for cap in (0, 1, full - 1):
        low = match.nnls_host(e["D"], e["S"][:, 3], 0, reg=e["reg"], chi2=e["chi2"], _max_evals=cap)
        assert low.status == 3 and low.evals == cap and (low.weights >= 0).all()
        assert 1 <= low.chi2 < e["chi2"] * (1 - cc.RTOL) and low.mu >= mu0 * (1 - 1e-15)       # the largest Jd <= T so far
    assert match.nnls_host(e["D"], e["S"][:, 3], 0, reg=e["reg"], chi2=e["chi2"], _max_evals=full).status == 0
    # an inner fit that hits its cap of solves ends the search as status 3 at the last good point; the baseline's own cap passes through
    low = match.nnls_host(e["D"], e["S"][:, 3], 0, reg=e["reg"], chi2=e["chi2"], _cap=1)
    assert low.status in (1, 3) and (low.weights >= 0).all()


def test_arguments():
    from epgpy_amd import match
    c = CASES["axis_first"]
    for bad in (1.0, 0.5, np.inf, np.nan, -2.0, [1.02], True):
        with pytest.raises(ValueError, match="chi2"):
            match.nnls_host(c["D"], c["S"], c["axis"], chi2=bad)
    for bad in (0.0, 1.0, -1e-3, np.nan, [1e-3]):
        with pytest.raises(ValueError, match="chi2_rtol"):
            match.nnls_host(c["D"], c["S"], c["axis"], chi2=1.02, chi2_rtol=bad)
    with pytest.raises(ValueError, match="reg"):
        match.nnls_host(c["D"], c["S"], c["axis"], reg=0.0, chi2=1.02)
    match.nnls_host(c["D"], c["S"], c["axis"], reg=0.0)      # (reg = 0 stays fine without chi2)

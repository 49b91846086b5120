"""CPU: `match.refine_host`, the NumPy statement of the formulas of `match.refine`, against the extended-precision yardstick of
tests/refine_cases.py on every case of the GPU test; the two caps that keep that test meaningful (decisive voxels, residual
bounds that are not vacuous) shown with the yardstick alone; the boundary (header, binding, ABI 11); the argument errors of
`refine` that need no device; and the point of it all on the analytic decay dictionary: one step from the matched atom lands
closer to the truth than the grid does."""
import os
import re

import numpy as np
import pytest

from epgpy_amd import _build, _lib, match
from tests import refine_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = rc.cases()


def host(case, **kw):
    J = case["J"] if "rows" not in case else case["J"][:, :, case["rows"]]
    return match.refine_host(case["D"], J, case["S"], case["index"], **kw)


@pytest.mark.parametrize("name", sorted(CASES))
def test_host_against_yardstick_and_caps(name):
    case = CASES[name]
    y = rc.yardstick(case)
    free = host(case)
    if "limit" in case:
        got = host(case, limit=case["limit"])
        clipped = np.any(got.delta != free.delta, axis=1) & np.isfinite(free.delta).all(axis=1)
        assert clipped.any() and (~clipped & np.isfinite(free.delta).all(axis=1)).any(), "some steps clipped and some not"
        worst = y.check(got.delta, got.scale, got.score, unclipped=free.delta, limit=case["limit"], what=name)
    else:
        worst = y.check(free.delta, free.scale, free.score, what=name)
    print(name, worst)
    assert worst["decisive"] >= 0.9, "at least 90 % of the voxels of every case are decisive"
    assert worst["sharp"] >= 0.9, "at least 90 % of the resolved voxels have a residual bound <= 1e-6 (sum |N||delta| + |y|)"


def test_cases_cover_the_slices():
    """a record count on each side of every slice boundary, and the counts and shapes the kernel's paths turn on"""
    nrecs = {c["D"].shape[0] for c in CASES.values()}
    assert {1, 2, 5, 37, 1000} <= nrecs
    for lo in (16, 32, 64):
        assert lo in nrecs and lo + 1 in nrecs and _lib.refine_slices(lo) * 2 == _lib.refine_slices(lo + 1)
    assert _lib.refine_slices(1) == 1 and _lib.refine_slices(1000) == 8
    assert {c["D"].shape[1] for c in CASES.values()} >= {1, 17, 257}
    assert {c["S"].shape[1] for c in CASES.values()} >= {1, 63, 64, 65, 131}
    assert {c["J"].shape[2] for c in CASES.values()} == {1, 2, 3, 4}


def test_special_voxels():
    case = CASES["special"]
    res = host(case)
    d = res.delta
    assert np.isnan(d[[0, 7]]).all() and (res.scale[[0, 7]] == 0).all() and (res.score[[0, 7]] == 0).all()        # index -1
    assert np.isfinite(d[[1, 11]]).all()                                                                         # atom 0
    assert np.isnan(d[[2, 8]]).all() and np.isnan(res.scale[[2, 8]]).all()                                        # the NaN atom
    assert np.isnan(d[[3, 9]]).all() and np.isnan(d[[5, 10]]).all() and np.isnan(d[6]).all()                      # built singular
    assert np.isnan(d[4]).all() and res.scale[4] == 0 and res.score[4] == 0                                       # all-zero signal
    assert np.isfinite(res.scale[[3, 5, 6]]).all() and (res.score[[3, 5, 6]] > 0).all()
    y = rc.yardstick(case)
    assert y.must_not[:11].all() or not y.must_resolve[[0, 2, 3, 4, 5, 6, 7, 8, 9, 10]].any()
    out = match.refine_host(case["D"], case["J"], case["S"][:, :3], np.array([17, -5, 1]))
    assert np.isnan(out.delta[:2]).all() and np.isfinite(out.delta[2]).all()


def test_boundary_agrees():
    """include/epgx.h, _lib.py, _build.py and the built library: the new entry point within ABI 11"""
    header = open(os.path.join(ROOT, "include", "epgx.h")).read()
    assert "#define EPGX_ABI_VERSION 11" in header and _lib.ABI_VERSION == 11
    proto = re.search(r"int epgx_signal_refine\(([^)]*)\)", header).group(1)
    assert len(proto.split(",")) == len(_lib.SYMBOLS["epgx_signal_refine"][1]) == 18
    lib = _lib.load()
    assert lib.epgx_abi_version() == 11 and hasattr(lib, "epgx_signal_refine")
    assert any(src == "epgx_refine.hip" for _, src, _ in _build.UNITS)
    for line in ("N_pq  = |rho|^2 Re(M_pq - conj(h_p) h_q / n)", "y_p   = Re(conj(rho) (b_p - rho conj(h_p)))",
                 "Nhat_pq = N_pq / (|rho|^2 sqrt(M_pp M_qq))", "score' = |num| / sqrt(den E)"):
        assert line in header and line in match.__doc__, line


def test_argument_errors_without_a_device():
    D, J, S, idx = rc.gaussian_case(5, 17, 9, 5, 2)
    D5 = np.concatenate([J, J, J[:, :, :1]], axis=2)
    with pytest.raises(NotImplementedError, match="1 .. 4"):
        match.refine(D, S, idx, jacobian=D5)
    with pytest.raises(ValueError, match="jacobian="):
        match.refine(D, S, idx)
    with pytest.raises(ValueError, match="shapes"):
        match.refine(D, S, idx, jacobian=J[:, :5])
    with pytest.raises(ValueError, match="not a column"):
        match.refine(D, S, idx, jacobian=J, variables=[0, 2])
    with pytest.raises(ValueError, match="twice"):
        match.refine(D, S, idx, jacobian=J, variables=[1, 1])
    with pytest.raises(NotImplementedError, match="1 .. 4"):
        match.refine(D, S, idx, jacobian=J, variables=[])
    with pytest.raises(ValueError, match="records"):
        match.refine(D, S[:4], idx, jacobian=J)
    for bad in (np.full(9, 17), np.full(9, -2)):
        with pytest.raises(ValueError, match="indices in"):
            match.refine(D, S, bad, jacobian=J)
    with pytest.raises(ValueError, match="shape"):
        match.refine(D, S, idx[:8], jacobian=J)
    with pytest.raises(ValueError, match="integer"):
        match.refine(D, S, idx.astype(float), jacobian=J)
    with pytest.raises(ValueError, match="grid"):
        match.refine(D, S, match.MatchResult(idx, None, None, (3, 3)), jacobian=J)
    for bad in (0.0, -1.0, [1.0, np.nan], [1.0, 2.0, 3.0]):
        with pytest.raises(ValueError, match="limit"):
            match.refine(D, S, idx, jacobian=J, limit=bad)
    for bad in (-1e-3, 1.0, np.nan):
        with pytest.raises(ValueError, match="rcond"):
            match.refine(D, S, idx, jacobian=J, rcond=bad)
        with pytest.raises(ValueError, match="rcond"):
            match.refine_host(D, J, S, idx, rcond=bad)


def test_estimate():
    D, J, S, idx = rc.gaussian_case(5, 12, 6, 5, 2)
    idx = idx.copy()
    idx[1] = -1
    res = match.refine_host(D.reshape(5, 3, 4), J.reshape(5, 3, 4, 2), S.reshape(5, 2, 3), idx.reshape(2, 3))
    assert res.grid == (3, 4) and res.delta.shape == (2, 3, 2) and res.variables == [0, 1]
    a, b = np.array([10.0, 20.0, 30.0])[:, None], np.array([1.0, 2.0, 3.0, 4.0])[None, :]
    est = res.estimate([a, b])
    assert est.shape == (2, 3, 2) and np.isnan(est[0, 1]).all()
    i, j = np.unravel_index(idx[0], (3, 4))
    assert est[0, 0, 0] == a[i, 0] + res.delta[0, 0, 0] and est[0, 0, 1] == b[0, j] + res.delta[0, 0, 1]
    with pytest.raises(ValueError):
        res.estimate([a])


def test_one_step_beats_the_grid():
    """noise-free signals between the grid rates of the analytic decay dictionary: |estimate - truth| < |grid value - truth| for
    every voxel off the grid.  65 rates from 0.02 to 0.6 are 5.5 % apart, so a voxel lies at most 2.7 % off its atom: there the
    linearisation error of one step, of second order in the offset, is far below the offset itself"""
    nrec, natoms = 37, 65
    rate = np.geomspace(0.02, 0.6, natoms)
    D, J = rc.decay_atoms(rate, nrec)
    frac = np.array([-0.45, -0.3, -0.1, 0.1, 0.3, 0.45])
    step = np.log(rate[1] / rate[0])
    truth = (rate[2:-2, None] * np.exp(frac[None, :] * step)).reshape(-1)
    S = (0.8 - 0.3j) * rc.decay_atoms(truth, nrec)[0]
    q = np.abs(np.conj(D).T @ S) ** 2 / (np.abs(D) ** 2).sum(axis=0)[:, None]
    index = np.argmax(q, axis=0)
    res = match.refine_host(D, J[:, :, :1], S, index)
    est = res.estimate([rate])[:, 0]
    assert np.isfinite(est).all()
    assert np.all(np.abs(est - truth) < np.abs(rate[index] - truth)), np.max(np.abs(est - truth) / np.abs(rate[index] - truth))
    assert np.all(res.score >= 1 - 1e-4)

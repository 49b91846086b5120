"""tests/hessian_recurrence.py pinned on the CPU: its float64 run reproduces the reference's own second derivatives (golden G13)
and every case of tests/hessian_cases.py has a float64 floor that leaves room for the 16 x bound of the device tests."""
import os

import numpy as np
import pytest

from epgpy_amd import epg
from tests import hessian_cases as hc
from tests import sequences as sq
from tests.hessian_recurrence import hessian_array, hessian_recurrence, pass_rows
from tests.jacobian_recurrence import column_errors

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "g13_hessian.npz")


@pytest.mark.parametrize("name", ["tutorial", "grid"])
def test_float64_recurrence_reproduces_the_reference(name):
    """the bar of test_g13_hessian_golden's data: 1e-12 absolute on every probe of the case (Hessians, the Jacobian, Z0)"""
    g = np.load(GOLDEN)
    tuples, opts = hc.g13_tuples(name)
    probes = next(p for n, _, p, _ in sq.hessian_cases(epg) if n == name)
    for i, pb in enumerate(probes):
        want = g[f"{name}_{i}"]
        if isinstance(pb, epg.Hessian):
            pairs = pb.pairs() + [(v, v) for v in pb.first_order()]
            res = hessian_recurrence(tuples, pairs, probe=pb.probe, dtype=np.complex128, **opts)
            got = hessian_array(res, pb.variables1, pb.variables2)
        else:
            names = [v for v in pb.variables if v != "magnitude"]
            res = hessian_recurrence(tuples, [(v, v) for v in names], probe=pb.probe, dtype=np.complex128, **opts)
            got = np.stack([res["S"] if v == "magnitude" else res["first"][v] for v in pb.variables], axis=-1)
        assert got.shape == want.shape, (name, i, got.shape, want.shape)
        err = float(np.max(np.abs(got - want)))
        print(name, i, "max abs error", err)
        assert err <= 1e-12, (name, i, err)
        if isinstance(pb, epg.Hessian):      # the float64 floor of every entry column, recorded in hessian_cases.FLOORS
            hi = hessian_array(hessian_recurrence(tuples, pairs, probe=pb.probe, dtype=np.clongdouble, **opts), pb.variables1, pb.variables2)
            floor = max(hc.entry_errors(got, hi))
            print(name, i, "floor", floor, "recorded", hc.FLOORS[f"g13_{name}"])
            assert floor <= hc.FLOORS[f"g13_{name}"] and hc.MARGIN * hc.FLOORS[f"g13_{name}"] <= hc.CAP


@pytest.mark.parametrize("name", sorted(hc.CASES))
def test_float64_floor(name):
    """per row of the pass: max|f64 - longdouble| / max|row| stays below the recorded floor, and 16 x floor below 1e-11"""
    c = hc.CASES[name]
    kw = dict(probe=c["probe"], max_nstate=c["cap"], through_plain=c["exact"], shape=c["shape"])
    lo = hessian_recurrence(c["tuples"], [c["pair"]], dtype=np.complex128, **kw)
    hi = hessian_recurrence(c["tuples"], [c["pair"]], dtype=np.clongdouble, **kw)
    errs = column_errors(pass_rows(lo, *c["pair"]), pass_rows(hi, *c["pair"]))
    print(name, "floor", max(errs), "recorded", hc.FLOORS[name])
    assert max(errs) <= hc.FLOORS[name]
    assert hc.MARGIN * hc.FLOORS[name] <= hc.CAP
    assert np.max(np.abs(pass_rows(hi, *c["pair"])[..., -1])) > 0        # the H row of every case is exercised

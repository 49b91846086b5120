"""CPU: the partial derivatives of the exchange operator (epgpy_amd/exchange.py) and the recurrence the device kernel is
held to (tests/exchange_jacobian_recurrence.py).

  1. every table of exchange_operator_partials against an independent extended-precision oracle: np.clongdouble, scaling and
     squaring of the Taylor series of the block matrix [[A tau, E tau], [0, A tau]], whose upper right block is the Frechet
     derivative.  Bound per table: 16 x floor x max|ref|, floor = what the value tables (mT, mL) of the same case achieve
     against the same oracle -- measured here and printed;
  2. identities: d/dtau = A m; khi = 0 gives the relaxation partials of E per compartment; coefficient arrays select
     compartments; dkhi= of a scalar-rate X equals the default;
  3. the recurrence with derivative states: float64 against clongdouble gives the per-case FLOORS, and its derivative agrees
     with Richardson central differences of the PLAIN recurrence (tests/exchange_recurrence.py) to 1e-9 per column;
  4. the interface: order1 forms, refusals, the pass rule, _check_exchange."""
import numpy as np
import pytest

from epgpy_amd import epg, exchange, evolution, _lib
from epgpy_amd import functions as _functions
from tests import exchange_jacobian_recurrence as xj
from tests.exchange_jacobian_recurrence import fd_host_errors      # (tests/test_gpu_exchange_jacobian.py takes it from here)
from tests.exchange_recurrence import recurrence, conserving_khi

LD = np.clongdouble


# ------------------------------------------------------------------------------------------ 1. tables against the oracle
def expm_taylor(mat):
    """expm of a small clongdouble matrix: scaling and squaring of its Taylor series"""
    mat = np.asarray(mat, dtype=LD)
    norm = float(np.max(np.sum(np.abs(mat), axis=1)))
    s = max(0, int(np.ceil(np.log2(max(norm, 1e-300)))) + 4)
    a = mat / LD(2.0 ** s)
    term = np.eye(mat.shape[0], dtype=LD)
    total = term.copy()
    for j in range(1, 40):
        term = term @ a / LD(j)
        total = total + term
    for _ in range(s):
        total = total @ total
    return total


def oracle(a, e):
    """(expm(a), Frechet derivative of expm at a along e) from the block matrix.  The derivative is linear in e, so the block
    carries e / max|e| and the result is scaled back: the number of squarings then follows the norm of `a` alone.  With e as it
    stands (max|e| = 5e4 for d/dT2 of a pool with T2 = 10 us) the squarings lose what extended precision gains: the oracle's
    own results for e and 5e4 e differed by 1.1e-14 relative, by 9e-16 at max|e| = 31 -- more than the bound they are to check."""
    n = a.shape[0]
    size = float(np.max(np.abs(e)))
    blk = np.zeros((2 * n, 2 * n), dtype=LD)
    blk[:n, :n] = blk[n:, n:] = a
    blk[:n, n:] = e / LD(size) if size > 0 else e
    out = expm_taylor(blk)
    return out[:n, :n], out[:n, n:] * LD(size)


def table_cases():
    """name -> (tau, khi, T1, T2, g, dkhi): compartments on axis 0, scalars per compartment"""
    rng = np.random.default_rng(11)
    out = {}
    for n in (2, 3, 4):
        T1, T2 = rng.uniform(300, 1500, n), rng.uniform(10, 150, n)
        out[f"n{n}_hermitian"] = (5.0, exchange.exchange_matrix(0.04, ncomp=n), T1, T2, None, exchange.exchange_matrix(1.0, ncomp=n))
        dens = rng.uniform(0.2, 1.0, n)
        khi = conserving_khi(rng, dens, 0.03)
        out[f"n{n}_densities_g"] = (4.0, khi, T1, T2, rng.uniform(-0.05, 0.05, n), khi / 0.03)
    out["khi_zero"] = (5.0, np.zeros((3, 3)), [900.0, 600.0, 300.0], [80.0, 40.0, 20.0], [0.01, 0.0, -0.02], exchange.exchange_matrix(1.0, ncomp=3))
    out["degenerate"] = (5.0, np.zeros((3, 3)), [900.0] * 3, [50.0] * 3, [0.01] * 3, exchange.exchange_matrix(1.0, ncomp=3))
    out["nearly_degenerate"] = (5.0, np.zeros((2, 2)), [900.0, 900.0], [50.0, 50.0 * (1 + 1e-9)], None, exchange.exchange_matrix(1.0))
    out["nearly_degenerate_khi"] = (5.0, exchange.exchange_matrix(1e-10), [900.0, 900.0], [50.0, 50.0 * (1 + 1e-9)], None, exchange.exchange_matrix(1.0))
    dens = np.array([0.85, 0.15])
    out["mt_stiff"] = (5.0, exchange.exchange_matrix(0.03, densities=dens), [1000.0, 1000.0], [50.0, 0.01], None,
                       exchange.exchange_matrix(1.0, densities=dens))
    return out


def rel(got, ref):
    return float(np.max(np.abs(got.astype(LD) - ref))) / float(np.max(np.abs(ref)))


TABLE_RESULTS = {}


@pytest.mark.parametrize("name", list(table_cases()))
def test_partial_tables_against_extended_precision(name):
    tau, khi, T1, T2, g, dkhi = table_cases()[name]
    n = len(T1)
    T1, T2 = np.asarray(T1, dtype=float), np.asarray(T2, dtype=float)
    gg = np.zeros(n) if g is None else np.asarray(g, dtype=float)
    aT = (-np.asarray(khi, dtype=LD) + np.diag((-1 / T2.astype(LD)) + 2j * LD(np.pi) * gg.astype(LD))) * LD(tau)
    aL = (-np.asarray(khi, dtype=LD) - np.diag(1 / T1.astype(LD))) * LD(tau)
    mat = exchange.exchange_operator(tau, khi, axis=0, T1=T1, T2=T2, g=g)
    floor = max(rel(mat[..., 0], oracle(aT, 0 * aT)[0]), rel(mat[..., 2].real, oracle(aL, 0 * aL)[0]), 2.0 ** -53)
    got = exchange.exchange_operator_partials(tau, khi, axis=0, T1=T1, T2=T2, g=g, dkhi=dkhi)
    worst = {}

    def compare(label, table, a, e):
        ref = oracle(a, e)[1]
        if float(np.max(np.abs(ref))) == 0:
            assert not np.any(table), label
            return
        worst[label] = rel(table, ref)

    zero = np.zeros((n, n), dtype=LD)
    compare("tau mT", got["tau"][0], aT, aT / LD(tau))
    compare("tau mL", got["tau"][1], aL, aL / LD(tau))
    compare("khi mT", got["khi"][0], aT, -np.asarray(dkhi, dtype=LD) * LD(tau))
    compare("khi mL", got["khi"][1], aL, -np.asarray(dkhi, dtype=LD) * LD(tau))
    for c in range(n):
        unit = zero.copy()
        unit[c, c] = 1
        compare(f"T2_{c} mT", got["T2"][0][c], aT, unit * LD(tau) / T2.astype(LD)[c] ** 2)
        compare(f"g_{c} mT", got["g"][0][c], aT, unit * LD(tau) * 2j * LD(np.pi))
        compare(f"T1_{c} mL", got["T1"][1][c], aL, unit * LD(tau) / T1.astype(LD)[c] ** 2)
        assert not np.any(got["T2"][1][c]) and not np.any(got["g"][1][c]) and not np.any(got["T1"][0][c])
    TABLE_RESULTS[name] = (floor, max(worst.values()))
    print(name, "floor of the value tables", floor, "worst partial table", max(worst, key=worst.get), max(worst.values()))
    assert max(worst.values()) <= 16 * floor, (name, floor, worst)


# ------------------------------------------------------------------------------------------------------- 2. identities
def test_tau_partial_is_generator_times_operator():
    tau, khi, T1, T2, g, _ = table_cases()["n3_densities_g"]
    got = exchange.exchange_operator_partials(tau, khi, axis=0, T1=T1, T2=T2, g=g, only={"tau"})["tau"]
    mat = exchange.exchange_operator(tau, khi, axis=0, T1=T1, T2=T2, g=g)
    aT = -khi + np.diag(-1 / T2 + 2j * np.pi * g)
    aL = -khi - np.diag(1 / T1)
    assert np.max(np.abs(got[0] - aT @ mat[..., 0])) <= 1e-15 and np.max(np.abs(got[1] - (aL @ mat[..., 2]).real)) <= 1e-15
    assert set(exchange.exchange_operator_partials(tau, khi, axis=0, T1=T1, T2=T2, g=g, only={"tau"})) == {"tau"}


def test_khi_zero_partials_are_relaxation_partials():
    tau, T1, T2, g = 5.0, np.array([900.0, 600.0, 300.0]), np.array([80.0, 40.0, 20.0]), np.array([0.01, 0.0, -0.02])
    got = exchange.exchange_operator_partials(tau, np.zeros((3, 3)), axis=0, T1=T1, T2=T2, g=g, only={"tau", "T1", "T2", "g"})
    want = evolution.relaxation_partials(tau, T1, T2, g)
    for p in ("T1", "T2", "g"):
        dT = sum(got[p][0][c] for c in range(3))
        dL = sum(got[p][1][c] for c in range(3))
        assert np.max(np.abs(dT - np.diag(want[p][0][..., 0]))) <= 4e-16 * max(np.max(np.abs(dT)), 1e-300), p
        assert np.max(np.abs(dL - np.diag(want[p][0][..., 2].real))) <= 4e-16 * max(np.max(np.abs(dL)), 1e-300), p
        for c in range(3):          # one non-zero entry per compartment table
            assert np.count_nonzero(got[p][0][c]) + np.count_nonzero(got[p][1][c]) == 1
    assert np.max(np.abs(got["tau"][0] - np.diag(want["tau"][0][..., 0]))) <= 4e-16 * np.max(np.abs(got["tau"][0]))
    assert np.max(np.abs(got["tau"][1] - np.diag(want["tau"][0][..., 2].real))) <= 4e-16 * np.max(np.abs(got["tau"][1]))


def test_coefficient_arrays_select_compartments():
    kw = dict(T1=[900.0, 300.0], T2=[70.0, 15.0], g=[0.0, 0.02])
    per = exchange.X(5.0, 0.04, order1={"a": {"T2": [1.0, 0.0]}, "b": {"T2": [0.0, 1.0]}, "all": {"T2": 1}, "w": {"T2": [2.0, -3.0]}}, **kw)
    t = per._variable_tables()
    raw = per._partial_tables({"T2"})["T2"]
    assert raw.shape == (2, 1, 12) and all(tab.shape == (1, 12) for tab in t.values())
    assert np.array_equal(t["a"], raw[0]) and np.array_equal(t["b"], raw[1])
    assert np.allclose(t["all"], raw[0] + raw[1], rtol=0, atol=1e-18) and np.allclose(t["w"], 2 * raw[0] - 3 * raw[1], rtol=0, atol=1e-18)
    assert per._variable_tables() is t                   # memoised
    # a coefficient that varies along another grid axis widens the table
    wide = exchange.X(5.0, 0.04, order1={"a": {"T2": [[1.0, 2.0, 3.0], [0.0, 0.0, 0.0]]}}, **kw)._variable_tables()["a"]
    assert wide.shape == (1, 3, 12) and np.array_equal(wide[0, 1], 2 * raw[0, 0])
    with pytest.raises(ValueError, match="compartment axis"):
        exchange.X(5.0, 0.04, order1={"a": {"tau": [1.0, 2.0]}}, **kw)._variable_tables()


def test_dkhi_of_a_scalar_rate_is_the_default():
    kw = dict(T1=[900.0, 300.0], T2=[70.0, 15.0], order1={"k": {"khi": 1}})
    a = exchange.X(5.0, 0.04, **kw)._variable_tables()["k"]
    b = exchange.X(5.0, 0.04, dkhi=exchange.exchange_matrix(1.0), **kw)._variable_tables()["k"]
    assert np.array_equal(a, b) and np.any(a)


# ------------------------------------------------------------------------------------------------------- 3. recurrence
@pytest.mark.parametrize("name", list(xj.CASES))
def test_float64_floor_of_every_case(name):
    c = xj.CASES[name]()
    errs = xj.column_errors(xj.run_case(c), xj.run_case(c, LD))
    print(name, "float64 floor per column", errs)
    assert max(errs) <= xj.FLOORS[name], (name, errs)
    assert 16 * xj.FLOORS[name] <= 1e-12


def test_floor_table_names_every_case():
    assert set(xj.FLOORS) == set(xj.CASES)


def test_recurrence_derivative_equals_central_differences_of_the_plain_recurrence():
    ref = xj.fd_reference()
    plain = recurrence(xj.fd_sequence(xj.FD_POINT, order1=False), (2,), 1.0, 9, dtype=LD)
    assert np.array_equal(ref[..., 0], plain)            # the state row is the plain recurrence
    fd = xj.fd_jacobian(lambda seq: recurrence(seq, (2,), 1.0, 9, dtype=LD))
    errs = xj.column_errors(fd, ref[..., 1:])
    print("extended recurrence against Richardson differences of the plain one", dict(zip(xj.FD_VARIABLES, errs)))
    assert max(errs) <= 1e-9


def test_float64_finite_difference_error_is_what_the_device_check_uses():
    errs = fd_host_errors()
    print("float64 host finite differences against the extended derivative", dict(zip(xj.FD_VARIABLES, errs)))
    assert len(errs) == len(xj.FD_VARIABLES) and 0 < max(errs) <= 1e-8


# ------------------------------------------------------------------------------------------------------------- 4. API
def test_order1_forms_and_refusals():
    kw = dict(T1=[900.0, 300.0], T2=[70.0, 15.0])
    assert exchange.X.PARAMETERS_ORDER1 == {"tau", "khi", "T1", "T2", "g"}
    assert exchange.X(5.0, 0.04, order1=True, **kw).order1 == {p: {p: 1} for p in exchange.X.PARAMETERS_ORDER1}
    assert exchange.X(5.0, 0.04, order1="T1", **kw).order1 == {"T1": {"T1": 1}}
    assert exchange.X(5.0, 0.04, order1=["T1", "khi"], **kw).order1 == {"T1": {"T1": 1}, "khi": {"khi": 1}}
    assert exchange.X(5.0, 0.04, order1={"R": "T1"}, **kw).order1 == {"R": {"T1": 1}}
    assert not exchange.X(5.0, 0.04, **kw).order1
    with pytest.raises(ValueError, match="Unknown parameter"):
        exchange.X(5.0, 0.04, order1="alpha", **kw)
    khi = exchange.exchange_matrix(0.04, densities=[0.8, 0.2])
    with pytest.raises(ValueError, match="dkhi"):
        exchange.X(5.0, khi, order1="khi", **kw)
    with pytest.raises(ValueError, match="shape of khi"):
        exchange.X(5.0, khi, order1="khi", dkhi=np.ones((3, 3)), **kw)
    assert np.any(exchange.X(5.0, khi, order1="khi", dkhi=khi / 0.04, **kw)._variable_tables()["khi"])
    with pytest.raises(NotImplementedError, match="X"):
        exchange.X(5.0, 0.04, order1="T1", order2=True, **kw)
    with pytest.raises(TypeError):
        exchange.X(5.0, 0.04, order3=True, **kw)


def test_encoded_partials():
    c = xj.CASES["x_2_1_3"]()
    enc, records, _ = _functions.compile_sequence(c["seq"], None, options={"max_nstate": 9}, variables=c["variables"])
    arrays = enc.plan_arrays(64)
    ops, dops, coef = arrays["ops"], arrays["dops"], arrays["coef"]
    xs = [i for i in range(len(ops)) if ops[i]["opcode"] == _lib.OP_X]
    x = next(op for op in c["seq"] if isinstance(op, epg.X))
    assert len(xs) == 15 and arrays["n_vars"] == 3 and arrays["deriv_flags"] & _lib.PLAN_NO_FOLD
    for v, var in enumerate(c["variables"]):
        off, space = int(dops[xs[0]]["coef_off"][v]), int(dops[xs[0]]["space"][v])
        assert off >= 0 and space == int(ops[xs[0]]["space"])      # one entry per group, like the operator's own table
        assert np.array_equal(coef[off: off + 3 * 12].reshape(3, 1, 12), x._variable_tables()[var])
        assert all(int(dops[i]["coef_off"][v]) == off for i in xs)   # one table per variable, however often X appears
    ts = [i for i in range(len(ops)) if ops[i]["opcode"] == _lib.OP_T]
    assert all(int(dops[i]["coef_off"][v]) < 0 for i in ts for v in range(3))


def test_pass_rule():
    assert [_lib.max_vars_exchange(2, K) for K in (64, 128, 256, 512)] == [3, 1, 0, 0]
    assert [_lib.max_vars_exchange(n, 64) for n in (2, 3, 4, 5, 8)] == [3, 1, 1, 0, 0]
    assert _lib.max_vars_exchange(3, 128) == 0 and _lib.max_vars_exchange(4, 128) == 0


def test_check_exchange_outcomes():
    x = epg.X(5.0, 0.01, T1=[900.0, 300.0], order1="T1")
    seq = [epg.T(10, 90), x, epg.ADC]
    jac = epg.Jacobian(["magnitude", "T1"])
    _functions._check_exchange(seq, [jac], None, "host", [0])
    _functions._check_exchange(seq, [jac], None, "host", [0], "resident", None)
    _functions._check_exchange(seq, [], None, "host", [0])
    assert _functions.exchange_derivatives(seq) and not _functions.exchange_derivatives([epg.T(10, 90), epg.X(5.0, 0.01), epg.ADC])
    plain = [epg.T(10, 90), epg.X(5, 0.01), epg.ADC]
    with pytest.raises(NotImplementedError, match="X.*no operator of the sequence declares"):      # the pinned case
        _functions._check_exchange(plain, [epg.Jacobian("T2")], None, "host", [0])
    with pytest.raises(NotImplementedError, match="X.*T2"):
        _functions._check_exchange(seq, [epg.Jacobian(["T1", "T2"])], None, "host", [0])
    with pytest.raises(NotImplementedError, match="X.*Hessian"):
        _functions._check_exchange(seq, [epg.Hessian(["T1"])], None, "host", [0])
    with pytest.raises(NotImplementedError, match="X.*device"):
        _functions._check_exchange(seq, [jac], None, "device", [0])
    with pytest.raises(NotImplementedError, match="X.*one GPU"):
        _functions._check_exchange(seq, [jac], None, "host", [0, 1])
    for mode in ("stepwise", "stream"):
        with pytest.raises(NotImplementedError, match=f"X.*{mode}"):
            _functions._check_exchange(seq, [jac], None, "host", [0], mode, None)
    with pytest.raises(NotImplementedError, match="X.*callback"):
        _functions._check_exchange(seq, [jac], None, "host", [0], "auto", print)
    with pytest.raises(NotImplementedError, match="X.*init"):
        _functions._check_exchange(seq, [jac], object(), "host", [0])
    with pytest.raises(NotImplementedError, match="X"):
        x(epg.StateMatrix.__new__(epg.StateMatrix))       # op(sm) of an X with order1: refused before the state is touched
    with pytest.raises(NotImplementedError, match="X"):      # a second-order pass
        _functions.compile_sequence(seq, None, variables=["T1", "T1:T1"], hessian=("T1", "T1"), fuse=False, collapse=False)

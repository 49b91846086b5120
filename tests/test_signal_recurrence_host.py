"""CPU: the extended-precision plain-signal recurrence (tests/signal_recurrence.py) and the per-record / per-order checks built
on it (tests/signal_cases.py).

  * FLOORS is honest: for every case at least the float64 oracle's largest per-record (per-order) error against the
    recurrence, and at most twice it; 16 x floor stays within 2e-12;
  * the recurrence in float64 equals the oracle to a few ulp on every operator kind, and its final state is the oracle's;
  * a combined operator is its factors;
  * the checks reject planted errors that the whole-array `close` of tests/test_gpu_parity.py admits, and anything but an
    exact zero in an order that the sequence never populated."""
import numpy as np
import pytest

from oracle import epg_numpy as onp
from tests import signal_cases as sc
from tests.signal_recurrence import signal_recurrence, oracle_signal, record_errors, order_errors, half_of, factors

_HEAVY = {}


def measured(name):
    """(largest per-record error, largest per-order error or 0) of the float64 oracle on a case"""
    if name not in _HEAVY:
        c = sc.CASES[name]
        want, want_state = sc.reference(name)
        got, got_state = sc.reference(name, oracle=True)
        orders = max(order_errors(half_of(got_state), want_state)) if c["out"] else 0.0
        _HEAVY[name] = (max(record_errors(got, want)), orders)
    return _HEAVY[name]


OWN = [name for name, c in sc.CASES.items() if c["ref"] == name]


@pytest.mark.parametrize("name", OWN)
def test_floor_table_is_honest(name):
    rec, orders = measured(name)
    floor = max(rec, orders)
    print(name, "float64 floor: records", rec, "orders", orders, "table", sc.FLOORS[name])
    assert floor <= sc.FLOORS[name] <= 2 * floor, (name, floor, sc.FLOORS[name])
    assert sc.MARGIN * sc.FLOORS[name] <= sc.CAP, name


def test_floor_table_names_every_case_and_the_cases_every_kernel():
    assert set(sc.FLOORS) == set(OWN)
    assert {c["kernel"] for c in sc.CASES.values()} == set(sc.ALL_NAMES) and len(sc.ALL_NAMES) == 96
    for c in sc.CASES.values():
        assert sc.CASES[c["ref"]]["tuples"] is c["tuples"] and sc.CASES[c["ref"]]["K"] == c["K"]


def every_operator():
    T2, g = np.array([40.0, 70.0, 110.0]), np.array([0.0, 0.02, -0.01])
    return [("T", 60.0, 20.0), ("E", 4.0, 700.0, T2, g), ("ADC",), ("ADC", "Z0"), ("S", 1), ("P", 3.0, -0.015), ("T", 78.0, -30.0),
            ("S", 2), ("ADC", "F0", 33.0), ("S", -3), ("T", 40.0, 35.0), ("S", 2), ("ADC",), ("PD", np.array([0.5, 0.7, 0.9]), False),
            ("E", 6.0, 900.0, T2, 0), ("ADC", "Z0", 12.0), ("SPOILER",), ("ADC",), ("T", 30.0, 10.0), ("S", 1), ("ADC",), ("RESET",),
            ("ADC", "Z0"), ("T", 50.0, 90.0), ("S", 1), ("E", 3.0, 900.0, T2, g), ("T", 120.0, 0.0), ("S", 1), ("ADC",),
            ("PD", 0.8), ("T", 20.0, 0.0), ("S", -1), ("E", 3.0, 900.0, T2, 0), ("ADC",), ("ADC", "Z0")]


@pytest.mark.parametrize("cap", [None, 2])
def test_float64_recurrence_equals_the_oracle_and_its_final_state(cap):
    """float64 against float64: a few ulp per record and per order (the oracle multiplies a rotation out of three matrices, the
    recurrence writes its elements down); truncation on and off; then from the final state as a start state"""
    ops = every_operator()
    got, state = signal_recurrence(ops, max_nstate=cap, dtype=np.complex128, return_state=True)
    want, want_state = onp.simulate(ops, max_nstate=cap, return_states=True)
    assert state.shape == want_state.shape
    assert max(record_errors(got, want)) <= 8 * np.finfo(float).eps
    assert max(order_errors(half_of(state), want_state)) <= 8 * np.finfo(float).eps
    tail = [("T", 70.0, 15.0), ("S", 1), ("E", 3.0, 900.0, 80.0, 0), ("ADC",), ("S", -2), ("ADC", "Z0")]
    got2, state2 = signal_recurrence(tail, max_nstate=cap, init=want_state, shape=(3,), dtype=np.complex128, return_state=True)
    want2, want_state2 = onp.simulate(tail, max_nstate=cap, init=want_state, shape=(3,), return_states=True)
    assert max(record_errors(got2, want2)) <= 8 * np.finfo(float).eps
    assert max(order_errors(half_of(state2), want_state2)) <= 8 * np.finfo(float).eps


def test_extended_final_state_matches_the_oracle():
    c = sc.CASES["f_128_in_1"]
    flat = [t for t in factors(c["tuples"]) if t[0] not in ("R", "D")]
    start = sc.start_of(c)[1]
    _, state = signal_recurrence(flat, max_nstate=c["cap"], init=start, shape=(3,), return_state=True)
    _, want = onp.simulate(flat, max_nstate=c["cap"], init=start, shape=(3,), return_states=True)
    assert state.shape == want.shape and state.dtype == np.clongdouble
    assert max(order_errors(half_of(want), state)) <= 1e-14


def test_combined_operator_is_its_factors():
    e, t = ("E", 2.0, 800.0, np.array([50.0, 90.0]), 0.01), ("T", 50.0, 35.0)
    head, tail = [("T", 60.0, 20.0), ("S", 1)], [("S", 1), ("ADC",), ("ADC", "Z0")]
    a = signal_recurrence(head + [("C", [e, t, e])] + tail)
    b = signal_recurrence(head + [e, t, e] + tail)
    assert np.array_equal(a, b)
    assert np.array_equal(oracle_signal(head + [("C", [e, t, e])] + tail), onp.simulate(head + [e, t, e] + tail))


def test_default_arguments_leave_the_jacobian_recurrence_alone():
    from tests.jacobian_recurrence import jacobian_recurrence
    ops = every_operator()
    a = jacobian_recurrence(ops, [])
    b, _ = jacobian_recurrence(ops, [], return_state=True)
    assert a.dtype == b.dtype and np.array_equal(a, b)


# ------------------------------------------------------------------------------------------------ the checks bite
def decaying():
    """b_decay_60: 60 echoes with T2 between 20 and 60 ms"""
    want, state = sc.reference("b_decay_60")
    return want, state, sc.FLOORS["b_decay_60"]


def test_per_record_check_bites_where_close_does_not():
    from tests.test_gpu_parity import close
    want, _, floor = decaying()
    good = want.astype(np.complex128)
    sc.check_records("host", good, want, floor)
    last = float(np.max(np.abs(want[-1])))
    assert last < 0.01, last                        # a late record: 1e-13 absolute is its eleventh digit, 16 floors its fourteenth
    bad = good.copy()
    bad[-1, 0] += 1e-13
    close(bad, good, 1e-12)
    with pytest.raises(AssertionError):
        sc.check_records("host", bad, want, floor)
    # one repetition too many in a folded run, planted where the whole-array bound is blind: 400 echoes decay below 1e-12, and
    # the last ten records each come from one echo further on (a tenth off, relatively)
    T1, T2, _, _ = sc.tissue(1, 261, 5, t2=(20.0, 60.0))
    long = signal_recurrence(sc.cpmg(T1, T2, np.ones(5), [], 400, tau=2.5, alpha=180.0), max_nstate=20)   # (exact refocusing: T2 decay alone)
    good = long.astype(np.complex128)
    assert 0 < float(np.max(np.abs(long[-11]))) < 1e-12
    folded = good.copy()
    folded[-11:-1] = good[-10:]
    close(folded, good, 1e-12)
    sc.check_records("host", good, long, 1e-13)
    with pytest.raises(AssertionError):
        sc.check_records("host", folded, long, 1e-13)
    sc.MEASURED.pop("host", None)


def test_per_order_check_bites_where_close_does_not():
    from tests.test_gpu_parity import close
    want, state, floor = decaying()
    half = np.ascontiguousarray(half_of(state).astype(np.complex128))
    K = 128
    buf = np.zeros(half.shape[:-1] + (K,), dtype=np.complex128)
    buf[..., : half.shape[-1]] = half
    sc.check_orders("host", buf, state, floor)
    top = half.shape[-1] - 1
    scale = float(np.max(np.abs(half[..., top])))
    assert 0 < scale < 1e-2 * float(np.max(np.abs(half))), (scale, float(np.max(np.abs(half))))
    bad = buf.copy()
    bad[0, 0, top] += 1e-13
    close(bad, buf, 1e-12)
    if 1e-13 > sc.MARGIN * floor * scale:
        with pytest.raises(AssertionError):
            sc.check_orders("host", bad, state, floor)
    else:
        pytest.fail(f"the highest populated order ({scale}) is too large for the planted error to matter")
    # an order the sequence never populated holds exactly zero
    tiny = buf.copy()
    tiny[1, 2, top + 1] = 1e-300
    close(tiny, buf, 1e-12)
    with pytest.raises(AssertionError):
        sc.check_orders("host", tiny, state, floor)
    sc.MEASURED.pop("host", None)


def test_zero_record_must_be_exactly_zero():
    want, _ = sc.reference("b_stops_1")
    zero = [r for r in range(want.shape[0]) if not want[r].any()]
    assert zero                                      # the F0 probe behind the spoiler
    good = want.astype(np.complex128)
    sc.check_records("host", good, want, sc.FLOORS["b_stops_1"])
    bad = good.copy()
    bad[zero[0], 0] = 1e-300
    with pytest.raises(AssertionError):
        sc.check_records("host", bad, want, sc.FLOORS["b_stops_1"])
    sc.MEASURED.pop("host", None)

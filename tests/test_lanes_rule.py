"""The window of the one-voxel-per-lane growing kernel (rows_grow_lanes_kernel; lanes_plan, epgx_planner.cpp), checked on the
oracle's NumPy port alone -- no device code takes part.

Between two shifts the kernel keeps the orders 0 .. min(top, rem): `top` = the shifts so far (nothing above is populated),
`rem` = the shifts left before the last probe (nothing above can reach order 0: tests/test_reach_rule.py).  Orders above the
window are stale in the kernel, so a state matrix whose orders above min(top, rem) are overwritten with noise after EVERY
operator must give the same probes, bit for bit, as the unmodified run."""
import numpy as np
import pytest

from oracle import epg_numpy as onp
from oracle import workloads as ow
from tests.test_reach_rule import garbage, shifts_left


def run(ops, grid, max_nstate, dead=None, slack=0):
    rem = shifts_left(ops)
    states = np.zeros(grid + (1, 3), dtype=np.complex128)
    states[..., 0, 2] = 1.0
    signal, top = [], 0
    for i, op in enumerate(ops):
        sig, states = onp.simulate([op], shape=grid, max_nstate=max_nstate, init=states, return_states=True)
        signal += list(sig)
        top += 1 if op[0] == "S" else 0
        if dead is not None:
            n = (states.shape[-2] - 1) // 2
            keep = max(min(top, rem[i]) + slack, -1)
            rows = np.abs(np.arange(-n, n + 1)) > keep
            if rows.any():
                dead(states, rows)
    return np.asarray(signal)


def echo(T1, T2, adc=("ADC",)):
    return [("S", 1), ("E", 5.0, T1, T2, 0), ("T", 120.0, 0), ("S", 1), ("E", 5.0, T1, T2, 0)] + ([adc] if adc else [])


def sequences():
    T1, T2 = np.linspace(200, 3000, 3)[:, None], np.linspace(20, 300, 2)[None, :]
    exc = [("T", 90, 90)]
    out = {f"mse_{n}": ow.mse_tuples(T1, T2, necho=n) for n in (1, 2, 7, 8, 10, 11, 15, 16, 20, 23)}
    out["unprobed_tail"] = exc + echo(T1, T2) * 9 + echo(T1, T2, adc=None) * 10
    out["every_other_echo"] = exc + (echo(T1, T2, adc=None) + echo(T1, T2)) * 10
    alpha, TR = ow.mrf_trains(40)
    out["mrf_40"] = ow.mrf_tuples(T1, T2, 1.0, alpha, TR)
    return out


@pytest.mark.parametrize("name", sorted(sequences()))
def test_orders_above_the_window_never_reach_a_probe(name):
    ops = sequences()[name]
    want = run(ops, (3, 2), 63)
    assert want.shape[0] == sum(1 for op in ops if op[0] == "ADC")
    for seed in (1, 2):
        assert np.array_equal(run(ops, (3, 2), 63, garbage(seed)), want), seed


def test_the_window_is_tight():
    """one order fewer than the window keeps does change the signal: the check above is not vacuous"""
    T1, T2 = np.array([1000.0]), np.array([80.0])
    ops = ow.mse_tuples(T1, T2, necho=12)
    want = run(ops, (1,), 63)
    assert np.array_equal(run(ops, (1,), 63, garbage(3)), want)
    assert not np.array_equal(run(ops, (1,), 63, garbage(3), slack=-1), want)

"""The rule behind the capacities of rows_grow_kernel's ranges (grow_reach, epgx_planner.cpp), checked on the oracle's NumPy port
alone -- no device code takes part.

A launch whose only outputs are order-0 probes (F0 / Z0) needs, at a point of its sequence with `rem` shifts left before the
last probe, nothing of the orders above `rem`: a coefficient of order k gets to order 0 through k applications of S(+-1) and
through nothing else (T, E, P, spoilers and resets act on every order by itself).  So a state matrix whose orders above `rem`
are zeroed -- or overwritten with anything finite -- after every operator must give the SAME probes, bit for bit, as the
unmodified run.  `rem` counts every S(+-1) whatever its sign (an over-estimate is safe, an under-estimate is not: the last
test shows one failing)."""
import numpy as np
import pytest

from oracle import epg_numpy as onp


def random_sequence(rng, nops, grid):
    """T / E / S(+-1) / ADC (F0 and Z0) in random order from equilibrium, now and then a spoiler or a reset; ends with
    operators behind the last probe"""
    T1 = rng.uniform(200, 3000, grid)
    T2 = rng.uniform(20, 300, grid)
    ops = []
    for _ in range(nops):
        u = rng.random()
        if u < 0.28:
            ops.append(("T", float(rng.uniform(5, 180)), float(rng.choice([0.0, 90.0, rng.uniform(0, 360)]))))
        elif u < 0.52:
            ops.append(("E", float(rng.uniform(1, 20)), T1, T2, float(rng.choice([0.0, rng.uniform(-0.05, 0.05)]))))
        elif u < 0.80:
            ops.append(("S", 1 if rng.random() < 0.8 else -1))
        elif u < 0.95:
            ops.append(("ADC",) if rng.random() < 0.7 else ("ADC", "Z0"))
        elif u < 0.98:
            ops.append(("SPOILER",))
        else:
            ops.append(("RESET",))
    return ops


def shifts_left(ops):
    """rem[i] = the S operators behind operator i up to the last ADC (-1 behind the last ADC: nothing is needed there)"""
    last = max((i for i, op in enumerate(ops) if op[0] == "ADC"), default=-1)
    rem, left = [-1] * len(ops), 0
    for i in range(last, -1, -1):
        rem[i] = left
        if ops[i][0] == "S":
            left += 1
    return rem


def run(ops, grid, max_nstate, dead=None, slack=0):
    """the oracle's driver (epg_numpy.simulate) one operator at a time; dead(states, rows) rewrites the rows of the orders
    above rem + slack after every operator"""
    rem = shifts_left(ops)
    states = np.zeros(grid + (1, 3), dtype=np.complex128)
    states[..., 0, 2] = 1.0
    signal = []
    for i, op in enumerate(ops):
        sig, states = onp.simulate([op], shape=grid, max_nstate=max_nstate, init=states, return_states=True)
        signal += list(sig)
        if dead is not None:
            n = (states.shape[-2] - 1) // 2
            keep = max(rem[i] + slack, -1)
            rows = np.abs(np.arange(-n, n + 1)) > keep
            if rows.any():
                dead(states, rows)
    return np.asarray(signal)


def zero(states, rows):
    states[..., rows, :] = 0


def garbage(seed):
    rng = np.random.default_rng(seed)

    def fill(states, rows):
        shape = states[..., rows, :].shape
        states[..., rows, :] = rng.normal(size=shape) + 1j * rng.normal(size=shape)
    return fill


@pytest.mark.parametrize("seed", range(40))
def test_orders_above_the_remaining_shifts_never_reach_a_probe(seed):
    rng = np.random.default_rng(1000 + seed)
    grid = (int(rng.integers(1, 4)), int(rng.integers(1, 4)))
    ops = random_sequence(rng, int(rng.integers(10, 120)), grid)
    max_nstate = [None, 63, 10][seed % 3]
    want = run(ops, grid, max_nstate)
    assert np.array_equal(run(ops, grid, max_nstate, zero), want)
    assert np.array_equal(run(ops, grid, max_nstate, garbage(seed)), want)


@pytest.mark.parametrize("necho", [1, 2, 9, 20, 40])
def test_echo_train_tail(necho):
    """the multi-echo train of the benchmark (T | S T S ADC ...), with unprobed echoes behind the last ADC"""
    T1, T2 = np.linspace(200, 3000, 3)[:, None], np.linspace(20, 300, 4)[None, :]
    echo = [("E", 2.5, T1, T2), ("S", 1), ("T", 150.0, 0.0), ("E", 2.5, T1, T2), ("S", 1), ("ADC",)]
    ops = [("T", 90.0, 90.0)] + echo * necho + echo[:-1] * 3
    want = run(ops, (3, 4), 63)
    assert want.shape[0] == necho
    assert np.array_equal(run(ops, (3, 4), 63, zero), want)
    assert np.array_equal(run(ops, (3, 4), 63, garbage(necho)), want)


def test_the_rule_is_tight():
    """one order fewer than the rule keeps does change the signal: the check above is not vacuous"""
    T1, T2 = np.array([1000.0]), np.array([80.0])
    echo = [("E", 2.5, T1, T2), ("S", 1), ("T", 150.0, 0.0), ("E", 2.5, T1, T2), ("S", 1), ("ADC",)]
    ops = [("T", 90.0, 90.0)] + echo * 12
    want = run(ops, (1,), 63)
    assert np.array_equal(run(ops, (1,), 63, garbage(3)), want)
    assert not np.array_equal(run(ops, (1,), 63, garbage(3), slack=-1), want)

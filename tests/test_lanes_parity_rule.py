"""The parity rule of rows_grow_lanes_kernel_odd (epgx_lanes_odd_cells.h; LanesPlan::odd, epgx_planner.cpp), checked on the
oracle's NumPy port alone -- no device code takes part.

In a train that repeats S(+1) . [E T E] . S(+1) behind an excitation, F moves by two orders between two refocusing pulses, Z by
none, and a rotation mixes F+(k), F-(k), Z(k) of one k.  The F orders whose parity is that of the shifts so far, and the Z
orders that are odd, form a class that never reads the other one; the excitation enters it through the first shift and every
probe (F0 behind the trailing shift) reads it.  The kernel computes that class alone, so a state matrix whose OTHER class is
overwritten with noise after EVERY operator must give the same probes, bit for bit, as the unmodified run -- and noise in the
class the kernel keeps must not."""
import numpy as np
import pytest

from oracle import epg_numpy as onp
from oracle import workloads as ow
from tests.test_lanes_rule import echo

SEEDS = (1, 2)


def run(ops, grid, max_nstate, seed=None, live=False):
    """the signal of `ops`, one operator at a time; with a seed, noise after every operator in the dead class (live: in the
    class the kernel computes)"""
    rng = None if seed is None else np.random.default_rng(seed)
    states = np.zeros(grid + (1, 3), dtype=np.complex128)
    states[..., 0, 2] = 1.0
    signal, shifts = [], 0
    for op in ops:
        sig, states = onp.simulate([op], shape=grid, max_nstate=max_nstate, init=states, return_states=True)
        signal += list(sig)
        shifts += 1 if op[0] == "S" else 0
        if rng is not None:
            n = (states.shape[-2] - 1) // 2
            k = np.abs(np.arange(-n, n + 1))
            f_rows = (k % 2 != shifts % 2) != live      # dead: |k| is not congruent to the shifts so far
            z_rows = (k % 2 == 0) != live               # dead: |k| even
            for rows, cols in ((f_rows, slice(0, 2)), (z_rows, slice(2, 3))):
                if rows.any():
                    shape = states[..., rows, cols].shape
                    states[..., rows, cols] = rng.normal(size=shape) + 1j * rng.normal(size=shape)
    return np.asarray(signal)


def sequences():
    T1, T2 = np.linspace(200, 3000, 3)[:, None], np.linspace(20, 300, 2)[None, :]
    exc = [("T", 90, 90)]
    out = {f"mse_{n}": ow.mse_tuples(T1, T2, necho=n) for n in (1, 2, 7, 10, 11, 20, 23)}
    out["unprobed_tail"] = exc + echo(T1, T2) * 9 + echo(T1, T2, adc=None) * 10
    out["every_other_echo"] = exc + (echo(T1, T2, adc=None) + echo(T1, T2)) * 10
    return out


@pytest.fixture(scope="module")
def clean():
    return {name: run(ops, (3, 2), 63) for name, ops in sequences().items()}


@pytest.mark.parametrize("name", sorted(sequences()))
def test_the_other_parity_never_reaches_a_probe(clean, name):
    ops = sequences()[name]
    want = clean[name]
    assert want.shape[0] == sum(1 for op in ops if op[0] == "ADC") and np.abs(want).max() > 0.01
    for seed in SEEDS:
        assert np.array_equal(run(ops, (3, 2), 63, seed), want), seed


@pytest.mark.parametrize("name", ["mse_1", "mse_20", "every_other_echo"])
def test_the_kept_parity_does(clean, name):
    """the same noise in the class the kernel computes changes every probe: the check above is not vacuous"""
    got = run(sequences()[name], (3, 2), 63, SEEDS[0], live=True)
    assert got.shape == clean[name].shape and np.all(got != clean[name])

"""rows_grow_kernel runs each of its three ranges at the smallest of 16 / 32 / 64 orders per voxel that holds the orders which
can still reach an order-0 probe (grow_reach, epgx_planner.cpp; EPGX_REACH=0: at 16 / 32 / 64 as before).  Orders above the
number of shifts left before the last probe cannot influence it (tests/test_reach_rule.py), so the signals must be those of
EPGX_REACH=0 BIT FOR BIT, and agree with the oracle as everywhere else."""
import os
import subprocess
import sys

import numpy as np
import pytest

from epgpy_amd import epg
from oracle import epg_numpy as onp
from tests import reach_cases, sequences as sq

pytestmark = pytest.mark.gpu
TOL = 1e-12


def close(a, b, tol=TOL):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (a.shape, b.shape)
    err = float(np.max(np.abs(a - b))) if a.size else 0.0
    assert err <= tol * max(1.0, float(np.max(np.abs(b))) if b.size else 1.0), err


def test_reach_is_bit_identical_and_right(tmp_path):
    """every sequence of reach_cases.cases(): (a) np.array_equal with a child process that runs EPGX_REACH=0; (b) the oracle
    (the cases taken from grow_cases: stream mode, as in test_growing_state_matrix_phases)"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = str(tmp_path / "plain.npz")
    subprocess.run([sys.executable, os.path.join(root, "tests", "reach_cases.py"), out], check=True,
                   env=dict(os.environ, EPGX_REACH="0"), cwd=root, timeout=900)
    plain = np.load(out)
    got = reach_cases.run_all(epg)
    assert set(got) == set(plain.files) and len(got) > 160
    for name, (tuples, seq, kw) in reach_cases.cases(epg).items():
        assert got[name].shape == plain[name].shape and np.array_equal(got[name], plain[name]), name
        if tuples is None:
            want = epg.simulate(seq, mode="stream", **kw)
        else:
            want = onp.simulate(tuples, max_nstate=kw["max_nstate"])
        try:
            close(got[name], want)
        except AssertionError as exc:
            raise AssertionError(f"{name}: {exc}") from None


def test_a_train_without_a_probe():
    """simulate() refuses a sequence without a probe before anything is launched, as the reference does (functions.py:87):
    the library never sees such a list from equilibrium, and grow_reach leaves a list without a probe at 16 / 32 / 64.  The
    call must fail THAT way, with reach on, and leave the library usable"""
    T1, T2 = np.linspace(200, 3000, 7)[:, None], np.linspace(20, 300, 5)[None, :]
    seq = sq.to_ops(epg, [("T", 90, 90)] + reach_cases.echo(T1, T2, adc=None) * 20)
    with pytest.raises(ValueError, match="without at least one Probe"):
        epg.simulate(seq, max_nstate=63)
    close(epg.simulate(seq + [epg.ADC], max_nstate=63),
          onp.simulate([("T", 90, 90)] + reach_cases.echo(T1, T2, adc=None) * 20 + [("ADC",)], max_nstate=63))


def trace_of(seq, capfd, **kw):
    os.environ["EPGX_TRACE"] = "1"
    try:
        capfd.readouterr()
        epg.simulate(seq, **kw)
        return capfd.readouterr().err
    finally:
        del os.environ["EPGX_TRACE"]


def test_capacities_of_the_echo_trains(capfd):
    """The record list of an n-echo train is the excitation and n times ONE echo record with two shifts; echo e (1 ..) leaves
    2 e as the highest populated order and has 2 (n + 1 - e) shifts left before the last probe, its own included.  grow_split
    cuts behind echo 7 (14 <= 15) and echo 15 (30 <= 31) whatever n is; a range needs 1 + max min(2 e, 2 (n + 1 - e)) orders.

    20 echoes -- records: excitation, echo x 7 | x 8 | x 5.
        [0, 2): e = 1 .. 7:  min(2 e, 42 - 2 e) = 2 e <= 14               -> 15 orders -> 16
        [2, 3): e = 8 .. 15: min(..) = 16, 18, 20, 20, 18, 16, 14, 12     -> 21 orders -> 32
        [3, 4): e = 16 .. 20: min(..) = 42 - 2 e = 10, 8, 6, 4, 2         -> 11 orders -> 16 (64 before)
    9 probed echoes and 10 unprobed ones behind them (a train of 9 alone has 19 orders and runs at 32 on rows_kernel; with
    the tail the launch has 39 orders: 64) -- for the probed echoes n = 9: echo x 7 | x 2, then the unprobed echoes, which need
    nothing (they stand behind the last probe), cut where they outgrow 32.
        first range:  e = 1 .. 7: min(2 e, 20 - 2 e) = 2, 4, 6, 8, 10, 8, 6            -> 11 orders -> 16
        second range: e = 8, 9:   min(16, 4), min(18, 2); the unprobed echoes: nothing ->  5 orders -> 16 (32 before)
        third range:  unprobed echoes only                                             ->  0 orders -> 16 (64 before)"""
    T1, T2 = np.linspace(200, 3000, 15)[:, None], np.linspace(20, 300, 14)[None, :]   # (a grid no plan exists for yet)
    seen = trace_of(sq.mse_ops(epg, T1, T2), capfd, max_nstate=63)
    assert "rows_grow_kernel<1>" in seen, seen
    assert "run: 4 records: [0, 2) at 16 orders per voxel, [2, 3) at 32, the rest at 16" in seen, seen
    listed = [ln for ln in seen.splitlines() if "grow list" in ln]
    assert len(listed) == 4 and [ln.split(" x ")[1].split()[0] for ln in listed] == ["1", "7", "8", "5"], listed
    assert [("next phase" in ln) for ln in listed] == [False, False, True, True], listed
    import re

    tuples = sq.mse_tuples(T1, T2, necho=9) + reach_cases.echo(T1, T2, adc=None) * 10
    made = {id(t): sq.to_ops(epg, [t])[0] for t in tuples}          # (one operator object per distinct tuple, as reach_cases)
    seen = trace_of([made[id(t)] for t in tuples], capfd, max_nstate=63)
    assert "rows_grow_kernel<1>" in seen, seen
    caps = re.search(r"run: \d+ records: \[0, 2\) at (\d+) orders per voxel, \[2, \d+\) at (\d+), the rest at (\d+)", seen)
    assert caps and caps.groups() == ("16", "16", "16"), seen
    listed = [ln for ln in seen.splitlines() if "grow list" in ln]
    assert [ln.split(" x ")[1].split()[0] for ln in listed][:3] == ["1", "7", "2"], listed
    assert sum("next phase" in ln for ln in listed) == 2, listed

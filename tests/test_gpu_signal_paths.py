"""Every device path of the plain signal against the extended-precision recurrence (tests/signal_recurrence.py,
np.clongdouble), PER RECORD -- for every record r  max_vox|gpu[r] - ref[r]| <= 16 floor max_vox|ref[r]| -- and, where a state
is written, PER ORDER, with every order that the sequence never populated exactly zero up to the capacity.  `floor` is what the
float64 oracle itself achieves on that case (tests/signal_cases.py FLOORS, kept honest by
tests/test_signal_recurrence_host.py).  A bound scaled by the whole array hides the late records of a decaying train and
the high orders of a state.

Every case first asks the library which kernel it would launch (choose_kernel, csrc/epgx_planner.cpp) and asserts the exact name
BEFORE launching.  Without derivative states choose_kernel can return 96 names that the launch tables instantiate
(epgx_launch*.h, epgx_inst.hip, epgx_split.hip; tests/signal_cases.py ALL_NAMES), and the cases name every one of them:
  (a) rows_kernel<NSP, R, RUNS>: NSP 1 / 2 / 4, R 1 / 2 / 4 with and without RUNS, R 8 without      21
  (b) rows_grow_kernel<NSP>                                                                           3
  (c) run_contig_kernel<M, NSP, HAS_IN>: M 2 / 4 / 8 / 16                                            24
  (d) run_contig_grow_kernel<M, NSP>: M 2 / 4 / 8 / 16                                               12
  (e) run_split_kernel<4, NSP, false>, run_kernel<8, NSP, false> + run_split_kernel<4, NSP, true>     6
  (f) run_kernel<M, NSP, HAS_IN>: M 1 / 2 / 4 / 8 / 16, with a state output                          30
No name is left out.  From equilibrium run_contig_kernel<., ., false> and run_split_kernel<4, ., false> are reached only
with the measurement knobs EPGX_CGROW=0 EPGX_SPLIT_GROW=0 EPGX_ROWS=0 (the library reads them once per process): those 15
cases run in ONE fresh child process, which asserts the names itself; this process's environment never changes.
The op-by-op StateMatrix path launches one operator at a time and has no single name: it is compared through sm.states."""
import os
import subprocess
import sys

import numpy as np
import pytest

from epgpy_amd import epg
from tests import signal_cases as sc
from tests.signal_cases import CASES, MEASURED, check_records, check_orders, floor_of

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nmax over records / orders of max|gpu - extended reference| / max|ref record / order| per group:",
          {k: float(f"{v:.3g}") for k, v in sorted(MEASURED.items())})


_REF = {}


def reference(name):
    """(records, final state) of a case in extended precision, computed once per module and shared by the cases that run the
    same inputs on another kernel"""
    key = CASES[name]["ref"]
    if key not in _REF:
        _REF[key] = sc.reference(key)
    return _REF[key]


_FAULT = []          # the first launch that raised: nothing more is started on the device after it


def guarded(fn):
    """run device work; once a launch or a download has raised, every later case fails before it touches the device"""
    if _FAULT:
        pytest.fail(f"not run: an earlier launch failed ({_FAULT[0]!r})")
    try:
        return fn()
    except AssertionError:
        raise
    except Exception as exc:
        _FAULT.append(exc)
        raise


def expect(kernel):
    def want_name(name):
        assert name == kernel, (name, kernel)
    return want_name


HERE = [name for name, c in CASES.items() if not c["child"]]
CHILD = [name for name, c in CASES.items() if c["child"]]


@pytest.mark.parametrize("name", HERE)
def test_paths(name):
    c = CASES[name]
    _, records, half = guarded(lambda: sc.launch(c, expect(c["kernel"])))
    want, want_state = reference(name)
    floor = floor_of(c["ref"])
    check_records(c["group"], records, want, floor)
    if c["out"]:
        check_orders(c["group"], half, want_state, floor)


_CHILD = {}


def child_results(tmp_path_factory):
    """the records of the cases that need the measurement knobs: one fresh child process for all of them"""
    if not _CHILD:
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        out = str(tmp_path_factory.mktemp("signal") / "child.npz")

        def run():
            subprocess.run([sys.executable, os.path.join(root, "tests", "signal_cases.py"), out] + CHILD, check=True,
                           env=dict(os.environ, **sc.KNOBS), cwd=root, timeout=300)
            return dict(np.load(out))
        _CHILD.update(guarded(run))
    return _CHILD


@pytest.mark.parametrize("name", CHILD)
def test_paths_under_knobs(name, tmp_path_factory):
    c = CASES[name]
    records = child_results(tmp_path_factory)[name]       # (the child asserted c["kernel"] before it launched)
    check_records(c["group"], records, reference(name)[0], floor_of(c["ref"]))


def test_state_matrix_operator_by_operator():
    """the same operators applied one at a time to a StateMatrix (one launch each): the final state per order"""
    c = CASES["f_128_eq_1"]
    ops = [op for op, t in zip(sc.ops_of(c["tuples"]), c["tuples"]) if t[0] != "ADC"]

    def run():
        sm = epg.StateMatrix(shape=sc.grid_of_case(c), kvalue=c["kvalue"])
        for op in ops:
            sm = op(sm, inplace=True)
        return np.asarray(sm.states)
    states = guarded(run)
    _, want_state = reference("f_128_eq_1")
    assert states.shape == want_state.shape, (states.shape, want_state.shape)
    from tests.signal_recurrence import half_of
    check_orders("f", np.ascontiguousarray(half_of(states)), want_state, floor_of("f_128_eq_1"))

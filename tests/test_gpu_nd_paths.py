"""Every device path of integer n-D shifts and diffusion against the extended-precision recurrence (tests/nd_recurrence.py,
np.clongdouble), PER RECORD -- for every record r  max_vox|gpu[r] - ref[r]| <= 16 floor max_vox|ref[r]| -- and, where a state
is written, PER COORDINATE, with every stored order whose coordinate the reference does not hold, and every order from the
plan's row count up to the capacity, exactly zero.  `floor` is what the float64 oracle itself achieves on that case
(tests/nd_cases.py FLOORS, kept honest by tests/test_nd_recurrence_host.py); no case needs 16 x floor > 2e-12.  The whole-array
`close` of tests/test_gpu_parity.py admits an error in the third to sixth digit of a diffusion-weighted record or of an outer
coordinate; these bounds do not.

Every case first asks the library which kernel it would launch (choose_kernel, csrc/epgx_planner.cpp) and asserts the exact
name BEFORE launching:
  (a) rows_kernel<NSP, 1, false> at 13 .. 16 stored coordinates, 1 / 4 / 5 / 65 voxels; the same plans on run_kernel<1, NSP, false>
  (b) run_kernel<M, NSP, false>, M = 1, 2, 4, 8: filled to K - 3 .. K - 31 and just above K / 2, GS_CONJ sources on both sides
  (c) run_kernel<16, NSP, false>: the two-pass gather at 545 and 1013 stored coordinates
  (d) run_kernel<M, NSP, true> from a start state given with coords=, and <M, NSP, false> into a buffer pre-filled with 7 + 7i;
      mode="stream" and the operator-by-operator StateMatrix path through sm.states
  (e) diffusion: scalar, per-voxel field, tensors, with and without k=, one strongly attenuated case
  (f) vectorised shifts, D with a table per voxel class, a truncating box, SPOILER / RESET
simulate(mode="resident") and simulate(mode="stream") must both meet the bound of their case."""
import numpy as np
import pytest

from epgpy_amd import epg
from tests import nd_cases as nc
from tests.nd_cases import CASES, MEASURED, CLOSEST, FLOORS, check_records, check_coordinates

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nlargest |gpu - extended reference| / (floor x max|ref record / coordinate|) per group, and its case:",
          {k: (float(f"{v[0]:.3g}"), v[1]) for k, v in sorted(MEASURED.items())},
          "closest to its bound (error / bound):", {k: (float(f"{v[0]:.3g}"), v[1]) for k, v in sorted(CLOSEST.items())})


_REF = {}


def reference(name):
    """(records, final table) of a case in extended precision, computed once and shared by the cases with the same inputs"""
    key = CASES[name]["ref"]
    if key not in _REF:
        _REF[key] = nc.reference(key)
    return _REF[key]


_FAULT = []


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


@pytest.mark.parametrize("name", list(CASES))
def test_paths(name):
    c = CASES[name]
    _, records, half, coords = guarded(lambda: nc.launch(c, expect(c["kernel"])))
    want, table = reference(name)
    floor = FLOORS[c["ref"]]
    check_records(name, c["group"], records, want, floor)
    if c["out"]:
        check_coordinates(name, c["group"], half, nc.rows_on(table, coords, c["grid"]), floor)


EQUILIBRIUM = [name for name, c in CASES.items() if c["start"] is None and c["ref"] == name]


@pytest.mark.parametrize("name", EQUILIBRIUM)
def test_modes(name):
    """simulate() state-resident and per-timestep: both within the case's bound"""
    c = CASES[name]
    ops = nc.ops_of(c["tuples"])
    want, _ = reference(name)
    for mode in ("resident", "stream"):
        got = guarded(lambda: np.asarray(epg.simulate(ops, mode=mode, shape=c["grid"], **c["opts"])))
        check_records(f"{name}[{mode}]", c["group"], got.reshape(want.shape), want, FLOORS[name])


@pytest.mark.parametrize("name", [name for name, c in CASES.items() if c["start"] is not None])
def test_state_matrix_with_coords(name):
    """from a StateMatrix built with coords=: mode="stream" (records), and operator by operator (records through F0 / Z0 and
    the final sm.states on sm.coords, per coordinate; rows the reference does not hold exactly zero)"""
    c = CASES[name]
    states, coords = nc.start_of(c)
    want, table = reference(name)
    floor = FLOORS[name]
    ops = nc.ops_of(c["tuples"])

    def stream():
        sm = epg.StateMatrix(states, coords=coords, **c["opts"])
        return np.asarray(epg.simulate(ops, init=sm, mode="stream"))
    check_records(name + "[stream]", c["group"], guarded(stream).reshape(want.shape), want, floor)

    def stepwise():
        sm = epg.StateMatrix(states, coords=coords, **c["opts"])
        for op, t in zip(ops, c["tuples"]):
            if t[0] != "ADC":
                sm = op(sm, inplace=True)
        return np.asarray(sm.states), np.asarray(sm.coords)
    got, rows = guarded(stepwise)
    from tests.signal_recurrence import half_of
    check_coordinates(name + "[op by op]", c["group"], np.ascontiguousarray(half_of(got)), nc.rows_on(table, rows, c["grid"]), floor)

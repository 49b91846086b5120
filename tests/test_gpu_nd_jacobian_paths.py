"""First-order derivative plans that gather (integer n-D shifts, EPGX_OP_GS) or diffuse in n-D against the extended-precision
recurrence of tests/nd_jacobian_recurrence.py (np.clongdouble), PER COLUMN: for every variable v
max|gpu[..., v] - ref[..., v]| <= 16 floor max|ref[..., v]|, `floor` the error of the same recurrence run in float64
(tests/nd_jacobian_cases.py FLOORS, kept honest by tests/test_nd_jacobian_recurrence_host.py); a column whose reference is
identically zero must be exactly zero.  The code under test: deriv_kernel<M, NSP, V> lane-strided with has_nd
(gather_shift(ds[j]) and apply_D(ds[j]) under through_plain, csrc/epgx_deriv_kernels.hip.h, csrc/epgx_deriv_record.hip.h),
and the planner's tables.

Every case first asks the library which kernel it would launch and asserts the exact name BEFORE launching:
  (a) deriv_kernel<M, NSP, V>, M = 1, 2, 4, 8, from equilibrium: gather shifts, near-full and just above K / 2
  (b) deriv_kernel<16, NSP, 1>: the two-pass gather at 545 and 1013 stored coordinates
  (c) D in the walk (scalar with / without k=, field, tensors), each with exact=False and exact=True; one strongly attenuated
  (d) from a start state given with coords= on every coordinate of the box (the a.in load of the strided layout)
  (e) vectorised shifts, D with a table per voxel class, SPOILER / RESET      (f) 70 voxels at K = 64
  (g) simulate(): 3 + 2 passes at K = 256, one variable per pass at 1024, probe kinds, an unknown variable, out="device"
  (h) operator by operator: op(sm) over one case of (a), an exact=False and an exact=True case of (c) and one of (e);
      sm.order1[var].states per coordinate (S.__call__ -> diff.propagate_plain; D, SPOILER and RESET as plain operators)"""
import numpy as np
import pytest

from epgpy_amd import epg, _lib
from epgpy_amd import functions as _functions
from tests import nd_jacobian_cases as jc
from tests.nd_jacobian_cases import CASES, CLOSEST, FLOORS, MEASURED, check, check_coordinates
from tests.nd_jacobian_recurrence import nd_jacobian_recurrence

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nlargest per-column |gpu - extended reference| / (floor x max|ref column|) per group, and its case:",
          {k: (float(f"{v[0]:.3g}"), v[1]) for k, v in sorted(MEASURED.items())},
          "closest to its bound (error / bound):", {k: (float(f"{v[0]:.3g}"), v[1]) for k, v in sorted(CLOSEST.items())})


_REF = {}


def reference(name):
    """the extended-precision Jacobian of a case, computed once per module"""
    if name not in _REF:
        _REF[name] = jc.reference(name)
    return _REF[name]


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
    got = guarded(lambda: jc.launch(c, expect(c["kernel"])))
    check(name, c["group"], got, reference(name), FLOORS[name])


# ------------------------------------------------------------------------------------------------ (g) through simulate()
def planned_names(ops, chunks, grid, options, exact):
    """the kernel of every pass of simulate(): one plan per chunk of variables"""
    names = []
    ctx = _lib.get_context(0)
    for chunk in chunks:
        enc, _, _ = _functions.compile_sequence(ops, [epg.Jacobian(chunk)], options=options, variables=chunk, shape=grid)
        enc.deriv_flags |= _lib.DERIV_THROUGH_PLAIN_OPS if exact else 0
        K = enc.capacity()
        names.append(_lib.kernel_for(ctx, enc.device_plan(ctx, K), K))
    return names


def g_reference(name):
    tuples, variables, grid, opts, exact = jc.g_cases()[name]
    return nd_jacobian_recurrence(tuples, variables, shape=grid, kvalue=opts["kvalue"], max_nstate=opts["max_nstate"], through_plain=exact)


def test_passes_at_256_orders():
    """five variables at K = 256: passes of 3 + 2, with exact_partials"""
    tuples, var, grid, opts, exact = jc.g_cases()["g_passes_256"]
    ops = jc.ops_of(tuples)
    assert planned_names(ops, [var[:3], var[3:]], grid, opts, exact) == ["deriv_kernel<4, 1, 3>", "deriv_kernel<4, 1, 2>"]
    got = guarded(lambda: epg.simulate(ops, probe=epg.Jacobian(["magnitude"] + var), exact_partials=exact, shape=grid, **opts))
    check("g_passes_256", "g", np.asarray(got), g_reference("g_passes_256"), FLOORS["g_passes_256"])


def test_passes_at_1024_orders():
    """two variables at K = 1024: one per pass"""
    tuples, var, grid, opts, exact = jc.g_cases()["g_passes_1024"]
    ops = jc.ops_of(tuples)
    assert planned_names(ops, [[v] for v in var], grid, opts, exact) == ["deriv_kernel<16, 1, 1>"] * 2
    got = guarded(lambda: epg.simulate(ops, probe=epg.Jacobian(["magnitude"] + var), exact_partials=exact, shape=grid, **opts))
    check("g_passes_1024", "g", np.asarray(got), g_reference("g_passes_1024"), FLOORS["g_passes_1024"])


def test_probe_kinds_unknown_variable_and_device_rows():
    """a Z0 Jacobian and a plain F0 probe next to an F0 Jacobian on the same ADC (one voxel); an unknown variable is exactly
    zero; the rows of out="device" are those of the host result"""
    tuples, var, grid, opts, exact = jc.g_cases()["g_probes"]
    ops = jc.ops_of(tuples)
    assert planned_names(ops, [["T2", "B1"]], grid, opts, exact) == ["deriv_kernel<1, 0, 2>"]
    jac, sig, jz = guarded(lambda: epg.simulate(ops, probe=[epg.Jacobian(["magnitude"] + var), "F0", epg.Jacobian(["magnitude", "B1", "T2"], probe="Z0")],
                                                shape=grid, **opts))
    kw = dict(shape=grid, kvalue=opts["kvalue"], max_nstate=opts["max_nstate"])
    want = nd_jacobian_recurrence(jc.with_probe(tuples, "F0"), var, **kw)
    floor = FLOORS["g_probes"]
    jac = np.asarray(jac).reshape(want.shape)
    check("g_probes[F0]", "g", jac, want, floor)
    assert not jac[..., 2].any()
    check("g_probes[signal]", "g", np.asarray(sig).reshape(want.shape[:-1])[..., None], want[..., :1], floor)
    wz = nd_jacobian_recurrence(jc.with_probe(tuples, "Z0"), ["B1", "T2"], **kw)
    check("g_probes[Z0]", "g", np.asarray(jz).reshape(wz.shape), wz, floor)
    dev = guarded(lambda: epg.simulate(ops, probe=epg.Jacobian(["magnitude", "T2", "B1"]), out="device", shape=grid, **opts))
    rows = guarded(lambda: np.stack([np.asarray(dev.column(v).download()) for v in ("magnitude", "T2", "B1")], axis=-1))
    check("g_probes[device]", "g", rows.reshape(want.shape[:-1] + (3,)), want[..., [0, 1, 3]], floor)


# ------------------------------------------------------------------------------------------------ (h) operator by operator
@pytest.mark.parametrize("name", jc.H_CASES)
def test_operator_by_operator(name):
    """op(sm) over the case's operators: every final sm.order1[var].states laid out on its own coordinates, every stored
    coordinate bounded by its own maximum over voxels and components, coordinates the reference does not hold exactly zero.
    Through this path D attenuates the state and leaves the derivative states alone whatever the case's `exact` says
    (nd_jacobian_cases.H_EXACT, asserted from the code by the host test); a variable nothing declares after the last RESET has
    no derivative state left, or an all-zero one"""
    from tests.nd_recurrence import layout
    from tests.signal_recurrence import half_of
    c = CASES[name]
    want = jc.h_reference(name)

    def stepwise():
        sm = epg.StateMatrix(shape=c["grid"], **c["opts"])
        for op in jc.ops_of([t for t in c["tuples"] if t[0] != "ADC"]):
            sm = op(sm, inplace=True)
        return {var: (np.asarray(d.states), np.asarray(d.coords)) for var, d in (getattr(sm, "order1", None) or {}).items()}
    got = guarded(stepwise)
    # (op(sm) carries every variable the operators declare; the case's own are the ones bounded)
    for var in c["variables"]:
        if not want[var]:
            assert var not in got or not got[var][0].any(), var
            continue
        states, coords = got[var]
        states = states.reshape(states.shape[:-2] + (1,) * (len(c["grid"]) - (states.ndim - 2)) + states.shape[-2:])
        states = np.broadcast_to(states, c["grid"] + states.shape[-2:])
        check_coordinates(f"{name}[{var}]", "h", np.ascontiguousarray(half_of(states)), layout(want[var], coords, c["grid"]), jc.COORD_FLOORS[name])

"""Every device path of the first-order derivatives against the extended-precision recurrence (tests/jacobian_recurrence.py,
np.clongdouble), PER COLUMN: for every variable v  max|gpu[..., v] - ref[..., v]| <= 16 floor max|ref[..., v]|, where `floor`
is what the float64 oracle itself achieves on that case (tests/test_jacobian_recurrence_host.py FLOORS) -- the columns of a
Jacobian differ by five orders of magnitude, and a bound scaled by the whole array hides an error in a small one.

Every case first asks the library which kernel it would launch (choose_kernel, csrc/epgx_planner.cpp) and asserts the exact
name, so that a selection change that drops a path fails here by name:
  (a) deriv_kernel<M, NSP, V, CONTIG> from equilibrium     (b) deriv_kernel from a state input
  (c) packed_deriv_kernel<NSP, V, 16|32>                    (d) rows_deriv_kernel<NSP, 4, V>
  (e) drun_kernel<NSP, V, SHAPE, V0>                        (f) packed_dfold_kernel<V, 16|32>
  (g) passes of simulate() and probes"""
import re

import numpy as np
import pytest

from epgpy_amd import epg, _lib
from epgpy_amd import functions as _functions
from tests.jacobian_recurrence import jacobian_recurrence, grid_of
from tests.jacobian_cases import (CASES, DRUN_FOLD, DRUN_LOGD, MEASURED, check, deriv_name, floor_of, g_cases, ops_of,
                                  options_of)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nmax over columns of max|gpu - extended reference| / max|ref column| per group:",
          {k: float(f"{v:.3g}") for k, v in sorted(MEASURED.items())})


_REF = {}


def reference(name, init=None):
    """the extended-precision Jacobian of a case, computed once per module (a case has one start state: the name is the key)"""
    if name not in _REF:
        c = CASES[name]
        grid = grid_of([t[:-1] if isinstance(t[-1], dict) else t for t in c["tuples"]])
        kw = dict(probe=c["probe"], max_nstate=c["cap"], through_plain=c["exact"], shape=grid, kvalue=c["kvalue"] or 1.0)
        _REF[name] = jacobian_recurrence(c["tuples"], c["variables"], init=init, **kw)
    return _REF[name]


def ctx():
    return _lib.get_context(0)


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


def launch(c, want_name):
    return guarded(lambda: _launch(c, want_name))


def _launch(c, want_name):
    """one derivative plan as _simulate_jacobian drives it: compile with the case's variables, ask for the kernel, assert its
    name, launch, download -> [record, *grid, 1 + V]; with `head` the start state is prepared operator by operator"""
    ops = ops_of(c["tuples"])
    options = options_of(c)
    init = None
    if c["head"]:
        init = epg.StateMatrix(shape=grid_of([t[:-1] if isinstance(t[-1], dict) else t for t in c["tuples"]]))
        for op in ops_of(c["head"]):
            init = op(init, inplace=True)
    probe = epg.Jacobian(["magnitude"] + c["variables"], probe=c["probe"])
    enc, records, _ = _functions.compile_sequence(
        ops, [probe], options=options, variables=c["variables"], shape=init.shape if init is not None else None,
        nstate0=init.nstate if init is not None else 0, kspace0=init._kspace if init is not None else None, dense_start=init is not None)
    enc.deriv_flags |= _lib.DERIV_THROUGH_PLAIN_OPS if c["exact"] else 0
    K = enc.capacity(at_least=(init.nstate + 1) if init is not None else 0)
    state = None
    if init is not None:
        work = init.copy()
        work._broadcast_to(enc.grid)
        work._reserve(max(K, init._state.K))
        state, K = work._state, work._state.K
    plan = enc.device_plan(ctx(), K)
    if state is None and c["packed"] and enc.packable(derivatives=True):
        K = enc.packable(derivatives=True)
    assert K == c["K"], (K, c["K"])
    name = _lib.kernel_for(ctx(), plan, K, state_in=state)
    want_name(name)                                  # BEFORE the launch
    nrow = 1 + len(c["variables"])
    assert enc.n_adc == len(records) * nrow
    sig = _lib.DeviceBuffer(ctx(), 16 * enc.n_adc * enc.nvox)
    _lib.run(ctx(), plan, 0, plan.n_ops, 0, enc.nvox, state, None, K, sig.ptr.value, enc.nvox, 0)
    raw = sig.download(np.complex128, (len(records), nrow) + tuple(enc.grid))
    return np.moveaxis(raw, 1, -1), (init.states if init is not None else None)


def expect(kernel):
    def want_name(name):
        if isinstance(kernel, str):
            assert name == kernel, name
        elif kernel[0] == "split":       # three derivative states of folded runs: the last variable alone -- the launcher runs that
            # leg's run list in its DRUN_LAST shape (V0 = 2 in the name) --, then the first two
            m = re.fullmatch(r"drun_kernel<4, 1, (\d+), 2> \+ drun_kernel<4, 2, (\d+), 0>", name)
            assert m and m.group(1) == m.group(2) and int(m.group(1)) & DRUN_FOLD, name
        else:
            _, V, V0, fold, logd = kernel
            m = re.fullmatch(r"drun_kernel<(\d+), (\d+), (\d+), (\d+)>", name)
            assert m, name
            nsp, v, code, v0 = (int(x) for x in m.groups())
            assert (v, v0) == (V, V0) and bool(code & DRUN_FOLD) == fold, name
            assert nsp == (4 if code & (DRUN_FOLD | DRUN_LOGD) else 1), name
            if logd is not None:
                assert bool(code & DRUN_LOGD) == logd, name
    return want_name


@pytest.mark.parametrize("name", list(CASES))
def test_paths(name):
    c = CASES[name]
    got, init = launch(c, expect(c["kernel"]))
    check(c["group"], got, reference(name, init), floor_of(name))


# ------------------------------------------------------------------------------------------------ (g) passes and probes
def planned_names(ops, chunks, options=None):
    """the kernel of every pass of simulate(): one plan per chunk of variables"""
    names = []
    for chunk in chunks:
        enc, _, _ = _functions.compile_sequence(ops, [epg.Jacobian(chunk)], options=options or {}, variables=chunk)
        K = enc.capacity()
        plan = enc.device_plan(ctx(), K)
        names.append(_lib.kernel_for(ctx(), plan, enc.packable(derivatives=True) or K))
    return names


@pytest.mark.parametrize("nvar", [4, 5])
def test_passes_at_512_orders(nvar):
    """four and five variables at K = 512: passes of 3 + 1 and 3 + 2"""
    tuples, var, _ = g_cases()[f"g_passes_{nvar}"]
    ops = ops_of(tuples)
    assert planned_names(ops, [var[:3], var[3:]]) == [deriv_name(512, 1, 3, False), deriv_name(512, 1, nvar - 3, True)]
    got = guarded(lambda: epg.simulate(ops, probe=epg.Jacobian(["magnitude"] + var)))
    check("g", got, jacobian_recurrence(tuples, var, probe="F0"), floor_of(f"g_passes_{nvar}"))


def test_passes_at_1024_orders():
    """two variables at K = 1024: one per pass"""
    tuples, _, _ = g_cases()["g_passes_1024"]
    ops = ops_of(tuples)
    assert planned_names(ops, [["T2"], ["B1"]]) == [deriv_name(1024, 1, 1, True)] * 2
    got = guarded(lambda: epg.simulate(ops, probe=epg.Jacobian(["magnitude", "T2", "B1"])))
    check("g", got, jacobian_recurrence(tuples, ["T2", "B1"], probe="F0"), floor_of("g_passes_1024"))


def test_probe_kinds_unknown_variable_and_device_rows():
    """a Z0 Jacobian and a plain F0 probe next to an F0 Jacobian on the same ADC; an unknown variable is exactly zero; the rows
    of out="device" are those of the host result"""
    tuples, _, _ = g_cases()["g_probes"]
    ops = ops_of(tuples)
    assert planned_names(ops, [["T2", "g"]], {"max_nstate": 20}) == ["packed_deriv_kernel<2, 2, 16>"]
    jac, sig, jz = guarded(lambda: epg.simulate(ops, probe=[epg.Jacobian(["magnitude", "T2", "zzz", "g"]), "F0",
                                                            epg.Jacobian(["magnitude", "g", "T2"], probe="Z0")], max_nstate=20))
    want = jacobian_recurrence(tuples, ["T2", "zzz", "g"], probe="F0", max_nstate=20)
    floor = floor_of("g_probes")
    check("g", jac, want, floor)
    assert not jac[..., 2].any()
    check("g", sig[..., None], want[..., :1], floor)
    check("g", jz, jacobian_recurrence(tuples, ["g", "T2"], probe="Z0", max_nstate=20), floor)
    dev = guarded(lambda: epg.simulate(ops, probe=epg.Jacobian(["magnitude", "T2", "g"]), max_nstate=20, out="device"))
    rows = guarded(lambda: np.stack([np.asarray(dev.column(v).download()) for v in ("magnitude", "T2", "g")], axis=-1))
    check("g", rows, want[..., [0, 1, 3]], floor)

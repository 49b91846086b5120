"""Derivative states through exchange on the device: dxrun_kernel<NC, M, V> (csrc/epgx_dxrun_kernels.hip.h).

  * every instantiation against the extended-precision recurrence (tests/exchange_jacobian_recurrence.py), PER COLUMN:
    max|gpu[..., v] - ref[..., v]| <= 16 floor max|ref[..., v]|, floor = what the float64 recurrence achieves on the case
    (FLOORS); the kernel name is asserted through _lib.kernel_for BEFORE the launch;
  * two cross-checks that do not share the oracle: with khi = 0 the Jacobian equals that of the same train with E on the
    existing derivative kernels; central differences of the existing plain xrun_kernel path agree with the Jacobian;
  * passes of simulate(), Adc(reduce=) under a Jacobian, and what is refused."""
import numpy as np
import pytest

from epgpy_amd import epg, exchange, _lib, EpgxError
from epgpy_amd import functions as _functions
from tests import exchange_jacobian_recurrence as xj

pytestmark = pytest.mark.gpu

_FAULT = []          # the first launch that raised: nothing more is started on the device after it
_REF = {}


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


def reference(name):
    if name not in _REF:
        _REF[name] = xj.run_case(xj.CASES[name](), np.clongdouble)
    return _REF[name]


def launch(c):
    """one derivative plan as _simulate_jacobian drives it: compile, ask for the kernel, assert its name, launch, download ->
    [record, *grid, 1 + V]"""
    variables = c["variables"]
    probe = epg.Jacobian(["magnitude"] + variables)
    options = {"max_nstate": c["max_nstate"]} if c.get("max_nstate") else {}
    enc, records, _ = _functions.compile_sequence(c["seq"], None, options=options, variables=variables)
    enc.deriv_flags |= _lib.DERIV_THROUGH_PLAIN_OPS if c.get("exact") else 0
    assert enc.grid == tuple(c["grid"]) and enc.deriv_flags & _lib.PLAN_NO_FOLD
    K = enc.capacity()
    ctx = _lib.get_context(0)
    plan = enc.device_plan(ctx, K)
    name = _lib.kernel_for(ctx, plan, K)
    assert name == c["kernel"], name                  # BEFORE the launch
    nrow = 1 + len(variables)
    assert enc.n_adc == len(records) * nrow
    sig = _lib.DeviceBuffer(ctx, 16 * enc.n_adc * enc.nvox)
    _lib.run(ctx, plan, 0, plan.n_ops, 0, enc.nvox, None, None, K, sig.ptr.value, enc.nvox, 0)
    raw = sig.download(np.complex128, (len(records), nrow) + tuple(enc.grid))
    return np.moveaxis(raw, 1, -1)


def check(got, want, floor, what):
    errs = xj.column_errors(got, want)
    print(what, "per-column error", ["%.3g" % e for e in errs], "bound", 16 * floor)
    assert max(errs) <= 16 * floor, (what, errs, 16 * floor)


@pytest.mark.parametrize("name", [n for n in xj.CASES if n.startswith("x_")])
def test_every_instantiation_against_extended_recurrence(name):
    c = xj.CASES[name]()
    got = guarded(lambda: launch(c))
    check(got, reference(name), xj.FLOORS[name], name)


def test_foldable_relaxation_stays_a_stage():
    """an E next to a T inside an X plan with derivatives: no fused table, every relaxation a stage with its own partial"""
    c = xj.CASES["x_2_1_2"]()
    enc, _, _ = _functions.compile_sequence(c["seq"], None, variables=c["variables"])
    opcodes = [rec[0] for rec in enc.records]
    assert _lib.OP_T0 not in opcodes and opcodes.count(_lib.OP_E) == 25 and not enc.fuses and not enc.fuse_partials


def test_khi_zero_equals_relaxation_on_the_derivative_kernels():
    cx, ce = xj.CASES["khi0_x"](), xj.CASES["khi0_e"]()
    gx = guarded(lambda: launch(cx))
    jac = epg.Jacobian(["magnitude"] + ce["variables"])
    ge = guarded(lambda: epg.simulate(ce["seq"], probe=jac))
    check(gx, reference("khi0_x"), xj.FLOORS["khi0_x"], "khi0_x")
    want = reference("khi0_e")
    bound = 16 * xj.FLOORS["khi0_x"] + 16 * xj.FLOORS["khi0_e"]
    errs = xj.column_errors(gx, ge.reshape(gx.shape))
    print("X(khi = 0) against E per column", errs, "bound", bound)
    assert max(errs) <= bound and want.shape == gx.shape


def test_central_differences_of_the_plain_kernel():
    """the existing plain path (xrun_kernel, no derivative code) differentiated numerically: an offset or a conjugation that
    the recurrence shared with the kernel would show here"""
    from tests.test_exchange_partials_host import fd_host_errors
    host = fd_host_errors()
    seq = xj.fd_sequence(xj.FD_POINT)
    enc, _, _ = _functions.compile_sequence(xj.fd_sequence(xj.FD_POINT, order1=False), None)
    ctx = _lib.get_context(0)
    assert _lib.kernel_for(ctx, enc.device_plan(ctx, 64), 64) == "xrun_kernel<2, 1, false>"
    # (a probe= replaces the probe of every ADC: the F0 Jacobian for the train's ADCs, the Z0 Jacobian for its Adc("Z0"))
    jf, jz = guarded(lambda: epg.simulate(seq, probe=[epg.Jacobian(xj.FD_VARIABLES), epg.Jacobian(xj.FD_VARIABLES, probe="Z0")]))
    jac = np.where((np.arange(16) % 2 == 0)[:, None, None], jf, jz)
    fd = guarded(lambda: xj.fd_jacobian(lambda s: np.asarray(epg.simulate(s), dtype=np.clongdouble)))
    assert jac.shape == fd.shape == (16, 2, len(xj.FD_VARIABLES))
    for v, var in enumerate(xj.FD_VARIABLES):
        err = float(np.max(np.abs(fd[..., v] - jac[..., v])) / np.max(np.abs(jac[..., v])))
        print(var, "finite difference of xrun_kernel against the Jacobian", err, "bound", 10 * host[v])
        assert err <= 10 * host[v], (var, err, host[v])


def _train_128(order1):
    x = epg.X(3.0, 0.05, T1=[800.0, 300.0], T2=[60.0, 15.0], order1=order1)
    return [part for j in range(24) for part in (epg.T(20.0 + j, 90.0, order1={"alpha": {"alpha": 1}}), x, epg.ADC, epg.S(3))]


def test_two_passes_equal_single_variable_runs():
    """NC = 2 at 128 orders carries one derivative state: two variables are two passes, bit for bit the single runs"""
    assert _lib.max_vars_exchange(2, 128) == 1
    o1 = {"T1": {"T1": 1}}
    both = guarded(lambda: epg.simulate(_train_128(o1), probe=epg.Jacobian(["magnitude", "alpha", "T1"])))
    a = guarded(lambda: epg.simulate(_train_128(o1), probe=epg.Jacobian(["magnitude", "alpha"])))
    b = guarded(lambda: epg.simulate(_train_128(o1), probe=epg.Jacobian(["magnitude", "T1"])))
    assert both.shape == (24, 2, 3) and np.abs(both[..., 1]).max() > 0 and np.abs(both[..., 2]).max() > 0
    assert np.array_equal(both[..., :2], a) and np.array_equal(both[..., [0, 2]], b)


def test_reduce_over_the_compartment_axis():
    c = xj.CASES["x_2_1_2"]()
    jac = epg.Jacobian(["magnitude"] + c["variables"])
    full = guarded(lambda: epg.simulate(c["seq"], probe=jac))
    seq = [epg.Adc(reduce=0) if op is epg.ADC else op for op in c["seq"]]
    summed = guarded(lambda: epg.simulate(seq, probe=jac))
    assert full.shape == (12, 2, 3, 3) and summed.shape == (12, 3, 3)
    assert float(np.max(np.abs(summed - full.sum(axis=1)))) <= 4e-16 * float(np.max(np.abs(full)))
    check(full, reference("x_2_1_2"), xj.FLOORS["x_2_1_2"], "simulate x_2_1_2")


def test_refusals_name_x_and_the_limit():
    o1 = {"T1": {"T1": 1}}
    jac = epg.Jacobian(["magnitude", "T1"])
    long = [part for j in range(40) for part in (epg.T(20.0, 90.0), epg.X(3.0, 0.05, T1=[800.0, 300.0], order1=o1), epg.ADC, epg.S(4))]
    with pytest.raises(NotImplementedError, match=r"X \(exchange\).*161 phase states.*256 orders"):
        epg.simulate(long, probe=jac)
    x5 = epg.X(3.0, exchange.exchange_matrix(0.05, ncomp=5), T1=[800.0, 300.0, 500.0, 600.0, 700.0], order1=o1)
    with pytest.raises(NotImplementedError, match=r"X \(exchange\).*5 compartments.*at most 4"):
        epg.simulate([epg.T(20.0, 90.0), x5, epg.ADC], probe=jac)
    seq = _train_128(o1)[:16]
    with pytest.raises(NotImplementedError, match=r"X \(exchange\).*Hessian"):
        epg.simulate(seq, probe=epg.Hessian(["T1"]))
    with pytest.raises(NotImplementedError, match=r"X \(exchange\).*device"):
        epg.simulate(seq, probe=jac, out="device")
    with pytest.raises(NotImplementedError, match=r"X \(exchange\).*stepwise"):
        epg.simulate(seq, probe=jac, mode="stepwise")
    with pytest.raises(NotImplementedError, match=r"X \(exchange\).*init"):
        epg.simulate(seq, probe=jac, init=epg.StateMatrix(shape=(2,)))
    # the library itself: a state input, and a capacity beyond the rule
    enc, _, _ = _functions.compile_sequence(seq, None, variables=["T1"])
    ctx = _lib.get_context(0)
    plan = enc.device_plan(ctx, 64)
    assert _lib.kernel_for(ctx, plan, 64) == "dxrun_kernel<2, 1, 1>"
    with pytest.raises(EpgxError, match="dxrun_kernel<N, K / 64, V>"):
        _lib.kernel_for(ctx, plan, 256)
    st = _lib.DeviceState(ctx, enc.nvox, 64)
    with pytest.raises(EpgxError, match="a state in HBM"):
        _lib.kernel_for(ctx, plan, 64, state_in=st, state_out=st)

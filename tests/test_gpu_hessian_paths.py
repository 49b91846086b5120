"""Every instantiation of the fused second-order pass (hess_kernel<M, NSP, DIAG>, csrc/epgx_hess_kernels.hip.h) against the
extended-precision recurrence (tests/hessian_recurrence.py, np.clongdouble), PER ROW of the pass -- S, S_a, (S_b,) H_ab:
max|gpu - ref| <= 16 floor max|ref row|, floor = what the float64 recurrence achieves on the case (hessian_cases.FLOORS).
Every launch first asks the library which kernel it would run (choose_kernel) and asserts the exact name.

On the parent commit `simulate(..., probe=Hessian, mode="resident")` raises and no plan is named hess_kernel: all of this fails."""
import os

import numpy as np
import pytest

from epgpy_amd import epg, _lib, diff
from epgpy_amd import functions as _functions
from tests import hessian_cases as hc
from tests import sequences as sq
from tests.hessian_recurrence import hessian_recurrence, pass_rows
from tests.jacobian_recurrence import column_errors

pytestmark = pytest.mark.gpu

_FAULT = []          # the first launch that raised: nothing more is started on the device after it


def guarded(fn):
    if _FAULT:
        pytest.fail(f"not run: an earlier launch failed ({_FAULT[0]!r})")
    try:
        return fn()
    except (AssertionError, NotImplementedError):
        raise
    except Exception as exc:
        _FAULT.append(exc)
        raise


def kernel_names(seq, probes, **options):
    """{pair: kernel name} of the passes simulate(seq, probe=probes, mode="resident") runs, from choose_kernel (no launch)"""
    ctx = _lib.get_context(0)
    flat = _functions.flatten_sequence(seq)
    names = {}
    shape = options.pop("shape", None)
    for a, b in _functions.hessian_passes(flat, probes):
        variables = [a, diff.hessian_key(a, b)] if a == b else [a, b, diff.hessian_key(a, b)]
        enc, _, _ = _functions.compile_sequence(flat, probes, options=dict(options), variables=variables, fuse=False, collapse=False,
                                                hessian=(a, b), shape=shape)
        K = enc.capacity()
        names[a, b] = (_lib.kernel_for(ctx, enc.device_plan(ctx, K), K), K)
    return names


_REF = {}


def reference(name):
    if name not in _REF:
        c = hc.CASES[name]
        res = hessian_recurrence(c["tuples"], [c["pair"]], probe=c["probe"], max_nstate=c["cap"], through_plain=c["exact"], shape=c["shape"])
        _REF[name] = pass_rows(res, *c["pair"])
    return _REF[name]


def run_pass(c):
    """the rows of one pass through the public call: [record, *grid, 3 | 4]"""
    a, b = c["pair"]
    seq = hc.ops_of(c["tuples"])
    probes = [epg.Jacobian(["magnitude", a] + ([b] if a != b else []), probe=c["probe"]), epg.Hessian([a], [b], probe=c["probe"])]
    opts = {**({"max_nstate": c["cap"]} if c["cap"] else {}), **({"shape": c["shape"]} if c["shape"] else {})}
    names = kernel_names(seq, probes, **opts)
    assert list(names) == [(a, b)] and names[a, b] == (c["kernel"], c["K"]), (names, c["kernel"], c["K"])
    jac, hes = guarded(lambda: epg.simulate(seq, probe=probes, mode="resident", exact_partials=c["exact"], **opts))
    return np.concatenate([jac, hes[..., 0, :]], axis=-1), seq, opts


@pytest.mark.parametrize("name", sorted(hc.CASES))
def test_pass_against_extended_precision(name):
    c = hc.CASES[name]
    got, _, _ = run_pass(c)
    want = reference(name)
    assert got.shape == want.shape
    assert 5 <= int(np.prod(want.shape[1:-1])) <= 13
    assert np.max(np.abs(want[..., -1])) > 0
    hc.check(name, got, want, hc.FLOORS[name])


def test_term_selection_is_visible_in_the_numbers():
    """h_select: with the cross term (dE/dT2) S_b1 wrongly taken at the relaxations the H row would move by far more than the
    bound -- the reference recurrence with the pair added to the relaxation's order2 differs from the case's by > 1e-3 relative"""
    c = hc.CASES["h_select"]
    tuples = [t if t[0] != "E" else t[:-1] + ({**t[-1], "order2": t[-1]["order2"] + [("b1", "T2")]},) for t in c["tuples"]]
    other = pass_rows(hessian_recurrence(tuples, [c["pair"]]), *c["pair"])
    assert column_errors(other, reference("h_select"))[-1] > 1e-3


@pytest.mark.parametrize("name", ["h_64_pair", "h_128_diag", "h_select"])
def test_first_order_rows_equal_a_jacobian_run(name):
    """the S, S_a, S_b rows of a pass against a Jacobian run of the same sequence.  NOT bit for bit: the Jacobian run fuses
    E . T . E, folds relaxations and takes other kernels (drun / rows_deriv / deriv_kernel with the contiguous layout), the pass
    runs every operator as a stage -- the same recurrence in other association orders.  Bound: 16 x the case's floor per column."""
    c = hc.CASES[name]
    got, seq, opts = run_pass(c)
    a, b = c["pair"]
    jac = guarded(lambda: epg.simulate(seq, probe=epg.Jacobian(["magnitude", a] + ([b] if a != b else []), probe=c["probe"]), **opts))
    errs = column_errors(got[..., :-1], jac.astype(np.clongdouble))
    print(name, "pass rows against the Jacobian run", errs)
    assert max(errs) <= hc.MARGIN * hc.FLOORS[name]


@pytest.mark.parametrize("name", ["tutorial", "grid"])
def test_g13_resident_against_golden_and_stepwise(golden, name):
    """the G13 sequences under mode="resident": the reference's own numbers at 1e-12 absolute (test_g13_hessian_golden's data),
    and the operator-by-operator path of the same process at 16 x floor per entry column"""
    g = golden("g13_hessian")
    _, seq, probes, opts = next(c for c in sq.hessian_cases(epg) if c[0] == name)
    names = kernel_names(seq, probes, **opts)
    assert names and all(k.startswith("hess_kernel<1, ") and K == 64 for k, K in names.values()), names
    assert {k.endswith("true>") for (a, b), (k, _) in names.items() if a == b} <= {True}
    assert {k.endswith("false>") for (a, b), (k, _) in names.items() if a != b} <= {True}
    res = guarded(lambda: epg.simulate(seq, probe=probes, mode="resident", **opts))
    step = guarded(lambda: epg.simulate(seq, probe=probes, mode="stepwise", **opts))
    for i, (pb, arr) in enumerate(zip(probes, res)):
        want = g[f"{name}_{i}"]
        assert np.asarray(arr).shape == want.shape
        err = float(np.max(np.abs(arr - want)))
        print(name, i, "max abs error against the golden file", err)
        assert err <= 1e-12
        if isinstance(pb, epg.Hessian):
            errs = hc.entry_errors(arr, np.asarray(step[i]).astype(np.clongdouble))
            print(name, i, "entry errors against mode='stepwise'", errs)
            assert max(errs) <= hc.MARGIN * hc.FLOORS[f"g13_{name}"]


def test_auto_and_stepwise_are_unchanged():
    """mode="auto" keeps the operator-by-operator path for Hessian probes: the bits of mode="stepwise" """
    _, seq, probes, opts = next(c for c in sq.hessian_cases(epg) if c[0] == "grid")
    auto = guarded(lambda: epg.simulate(seq, probe=probes, **opts))
    step = guarded(lambda: epg.simulate(seq, probe=probes, mode="stepwise", **opts))
    assert all(np.array_equal(x, y) for x, y in zip(auto, step))


def test_what_the_fused_path_does_not_take_is_named():
    _, seq, probes, opts = next(c for c in sq.hessian_cases(epg) if c[0] == "tutorial")
    with pytest.raises(NotImplementedError, match="init"):
        epg.simulate(seq, probe=probes, mode="resident", init=[0, 0, 1])
    with pytest.raises(NotImplementedError, match="ngpu"):
        epg.simulate(seq, probe=probes, mode="resident", ngpu=2)
    with pytest.raises(NotImplementedError, match="callback"):
        epg.simulate(seq, probe=probes, mode="resident", callback=epg.PartialsPruner())
    with pytest.raises(NotImplementedError, match="stream"):
        epg.simulate(seq, probe=probes, mode="stream")
    long = [seq[0]] + seq[1:7] * 300            # 600 shifts: above 512 orders
    with pytest.raises(NotImplementedError, match="512"):
        epg.simulate(long, probe=probes, mode="resident")
    with pytest.raises(NotImplementedError, match="n-D shifts"):
        epg.simulate(seq[:-1] + [epg.S([1, 0]), epg.ADC], probe=probes, mode="resident")
    # an integer shift given as a NumPy integer is a 1-D shift
    res = guarded(lambda: epg.simulate([seq[0], epg.S(np.int64(1))] + seq[2:], probe=probes, mode="resident"))
    want = guarded(lambda: epg.simulate(seq, probe=probes, mode="resident"))
    assert all(np.array_equal(x, y) for x, y in zip(res, want))
    with pytest.raises(NotImplementedError, match="complex64"):
        epg.simulate(seq, probe=probes, mode="resident", dtype=np.complex64)
    with pytest.raises(NotImplementedError, match="equilibrium"):
        epg.simulate(seq, probe=probes, mode="resident", equilibrium=[0, 0, 0.5])
    with pytest.raises(NotImplementedError, match="float shift"):
        epg.simulate(seq[:-1] + [epg.S(0.5), epg.ADC], probe=probes, mode="resident", kgrid=0.25)
    with pytest.raises(NotImplementedError, match="X"):
        epg.simulate([epg.T(30.0, 0.0, order2="alpha"), epg.X(10, 0.1), epg.ADC], probe=epg.Hessian("alpha"),
                     mode="resident")
    from epgpy_amd import rfpulse
    pulse = rfpulse.RFPulse(np.hanning(8), 1.0, alpha=30.0)
    with pytest.raises(NotImplementedError, match="RFPulse"):
        epg.simulate([pulse] + seq, probe=probes, mode="resident")
    from epgpy_amd import distributed
    with pytest.raises(NotImplementedError, match="Hessian"):
        distributed.simulate_sharded(seq, probe=probes)


def _second_order_arrays():
    """the host arrays of a valid one-pair pass (G13 "grid", pair (T2, b1)), to be broken one field at a time"""
    _, seq, probes, opts = next(c for c in sq.hessian_cases(epg) if c[0] == "grid")
    enc, _, _ = _functions.compile_sequence(seq, probes, options=dict(opts), variables=["T2", "b1", diff.hessian_key("T2", "b1")],
                                            fuse=False, collapse=False, hessian=("T2", "b1"))
    return dict(enc.plan_arrays(64))


def _refused(arrays, code, text):
    ctx = _lib.get_context(0)
    with pytest.raises(_lib.EpgxError, match=text) as info:
        _lib.DevicePlan(ctx, **arrays)
    assert f"({code})" in str(info.value) or str(code) in str(info.value), str(info.value)


def test_plan_create_refuses_what_a_second_order_plan_cannot_carry():
    """epgx_plan_create on EPGX_DERIV_SECOND plans: every refusal with its code (-4 EPGX_ERR_UNSUPPORTED, -1 EPGX_ERR_INVALID) and a
    message that names the cause; the unbroken arrays are accepted and named hess_kernel"""
    good = _second_order_arrays()
    ctx = _lib.get_context(0)
    assert _lib.kernel_for(ctx, _lib.DevicePlan(ctx, **good), 64) == "hess_kernel<1, 1, false>"     # (one index space: the (T2, g) grid)
    _refused({**good, "deriv_flags": good["deriv_flags"] & ~_lib.PLAN_NO_FOLD}, -4, "EPGX_PLAN_NO_FOLD")
    _refused({**good, "n_vars": 1}, -1, "n_vars = 3")
    fuse = np.zeros(1, dtype=_lib.FUSE_DTYPE)
    _refused({**good, "fuse": fuse, "n_coef_generated": 12}, -4, "n_fuse")
    fp = np.zeros(1, dtype=_lib.FUSE_PARTIAL_DTYPE)
    _refused({**good, "fuse_partial": fp, "n_coef_generated": 14}, -4, "n_fuse_partial")
    step = np.zeros(1, dtype=_lib.CHAIN_STEP_DTYPE)
    _refused({**good, "chain": [(len(good["coef"]), -1, step)], "n_coef_generated": 14}, -4, "chains")
    ops = good["ops"].copy()
    t = int(np.flatnonzero(ops["opcode"] == _lib.OP_T)[0])
    ops[t]["opcode"], ops[t]["ncoef"] = _lib.OP_T0, 12
    _refused({**good, "ops": ops}, -4, "EPGX_OP_T0")
    dops = good["dops"].copy()
    e = int(np.flatnonzero(good["ops"]["opcode"] == _lib.OP_E)[0])
    dops[e]["reserved"] = _lib.HESS_CROSS_B            # the relaxation has no partial w.r.t. b1
    _refused({**good, "dops": dops}, -1, "cross-term bit")
    dops = good["dops"].copy()
    dops[e]["reserved"] = 4
    _refused({**good, "dops": dops}, -1, "cross-term bit")
    # a second-order plan above 512 orders, from a state, or with a state output is refused by epgx_run / epgx_kernel_for
    plan = _lib.DevicePlan(ctx, **good)
    with pytest.raises(_lib.EpgxError, match="second-order plans support K = 64, 128, 256, 512"):
        _lib.kernel_for(ctx, plan, 1024)

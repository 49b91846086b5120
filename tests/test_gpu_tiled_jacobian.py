"""GPU: Jacobians beyond 1024 orders on the tiled path (csrc/epgx_tiled.hip tiled_deriv_kernel, include/epgx.h
epgx_run_tiled_deriv), through epg.simulate(..., probe=Jacobian(...), mode="resident").

(a) every case of tests/tiled_jacobian_cases.py against the extended-precision recurrence, PER COLUMN, at 16 x the case's
    float64 floor -- the kernel name asked for and asserted before the launch;
(b) the same bits as the in-register path (deriv_kernel<16, ., 1, true>) on a plan that fits both;
(c) voxel slabs give the same bits; (d) the reference's own numbers (g23); (e) without mode="resident" the call still raises."""
import os
import subprocess
import sys

import numpy as np
import pytest

from epgpy_amd import epg, _lib
from epgpy_amd import functions as _functions
from tests import tiled_jacobian_cases as tc
from tests.jacobian_cases import MEASURED, check, ops_of
from tests.jacobian_recurrence import jacobian_recurrence, grid_of

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nmax over columns of max|gpu - extended reference| / max|ref column|:", {k: float(f"{v:.3g}") for k, v in sorted(MEASURED.items())})


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


def ctx():
    return _lib.get_context(0)


def start_state(c):
    """the start state of a case with a head, prepared operator by operator"""
    if not c["head"]:
        return None
    init = epg.StateMatrix(shape=grid_of(tc.plain(c["tuples"])))
    for op in ops_of(c["head"]):
        init = op(init, inplace=True)
    return init


_REF = {}


def reference(name, probe, init=None):
    if (name, probe) not in _REF:
        c = tc.CASES[name]
        _REF[name, probe] = jacobian_recurrence(c["tuples"], c["variables"], probe=probe, max_nstate=c["cap"], through_plain=c["exact"],
                                                shape=grid_of(tc.plain(c["tuples"])), init=init)
    return _REF[name, probe]


def assert_kernels(c, ops, init, chunks):
    """the kernel of every pass, from epgx_tiled_deriv_info -- BEFORE any launch of the case"""
    options = {"max_nstate": c["cap"]} if c["cap"] else {}
    for chunk in chunks:
        enc, _, _ = _functions.compile_sequence(ops, [epg.Jacobian(chunk)], options=options, variables=chunk, fuse=c["fuse"],
                                                shape=init.shape if init is not None else None,
                                                nstate0=init.nstate if init is not None else 0, dense_start=init is not None)
        assert enc.tiled_ok(derivatives=True) and enc.peak + 1 > _lib.MAX_DERIV_K
        top0 = init._state.K - 1 if init is not None else None
        info = _lib.tiled_deriv_info(ctx(), enc.device_plan(ctx()), enc.tiled_capacity(top0), top0 or 0)
        assert info["names"].split(" + ")[0] == f"tiled_deriv_kernel<8, 32, {len(chunk)}>", info
        assert info["peak"] // _lib.TILED_W >= 2, info                   # three tiles or more
        assert ("tiled_shift" in info["names"]) == (info["shifts"] > 0)


@pytest.mark.parametrize("name", [n for n in tc.CASES if n != "t_probes"])
def test_cases(name):
    c = tc.CASES[name]
    ops = ops_of(c["tuples"])
    init = guarded(lambda: start_state(c))
    V = _lib.TILED_DERIV_V
    chunks = [c["variables"][i:i + V] for i in range(0, len(c["variables"]), V)]
    guarded(lambda: assert_kernels(c, ops, init, chunks))
    columns = c["columns"] or ["magnitude"] + c["variables"]
    kw = dict(probe=epg.Jacobian(columns), mode="resident", exact_partials=c["exact"], fuse=c["fuse"], init=init)
    if c["cap"]:
        kw["max_nstate"] = c["cap"]
    got = guarded(lambda: epg.simulate(ops, **kw))
    want = reference(name, "F0", init.states if init is not None else None)
    if c["columns"]:          # an unknown variable: its column is exactly zero, the others are the plan's
        unknown = [i for i, v in enumerate(columns) if v != "magnitude" and v not in c["variables"]]
        assert unknown and all(not got[..., i].any() for i in unknown)
        got = got[..., [i for i in range(len(columns)) if i not in unknown]]
    check("tiled", got, want, tc.FLOORS[name])
    if name == "t_shifts":
        assert "tiled_shift" in _shift_names(c, ops)


def _shift_names(c, ops):
    enc, _, _ = _functions.compile_sequence(ops, [epg.Jacobian(c["variables"])], options={"max_nstate": c["cap"]}, variables=c["variables"])
    return _lib.tiled_deriv_info(ctx(), enc.device_plan(ctx()), enc.tiled_capacity())["names"]


def test_probe_kinds_and_device_rows():
    """a Z0 Jacobian and a plain F0 probe next to an F0 Jacobian on the same ADC; the rows of out="device" are the host result's bits"""
    c = tc.CASES["t_probes"]
    ops = ops_of(c["tuples"])
    guarded(lambda: assert_kernels(c, ops, None, [c["variables"]]))
    jac, sig, jz = guarded(lambda: epg.simulate(ops, probe=[epg.Jacobian(["magnitude", "T2", "B1"]), "F0",
                                                            epg.Jacobian(["magnitude", "B1", "T2"], probe="Z0")], mode="resident"))
    floor = tc.FLOORS["t_probes"]
    want = reference("t_probes", "F0")
    check("tiled", jac, want, floor)
    check("tiled", sig[..., None], want[..., :1], floor)
    check("tiled", jz, reference("t_probes", "Z0")[..., [0, 2, 1]], floor)
    dev = guarded(lambda: epg.simulate(ops, probe=epg.Jacobian(["magnitude", "T2", "B1"]), mode="resident", out="device"))
    assert type(dev).__name__ == "DeviceJacobian"
    rows = guarded(lambda: np.stack([np.asarray(dev.column(v).download()) for v in ("magnitude", "T2", "B1")], axis=-1))
    host = guarded(lambda: epg.simulate(ops, probe=epg.Jacobian(["magnitude", "T2", "B1"]), mode="resident"))
    assert np.array_equal(rows, host) and np.array_equal(np.asarray(dev), host)
    with pytest.raises(NotImplementedError):      # more variables than one pass holds: the existing error
        epg.simulate(ops, probe=epg.Jacobian(["magnitude", "T1", "T2", "B1"]), mode="resident", out="device")


# ------------------------------------------------------------------ (b) the bits of the in-register path
def test_same_bits_as_deriv_kernel():
    """one variable, 901 orders: deriv_kernel<16, 1, 1, true> through epgx_run and three tiles through epgx_run_tiled_deriv walk
    the same record body on the same per-order arithmetic"""
    T1, T2, B1 = tc.tissue(2310)
    exc, rfc, rlx = tc.stages(2310)
    tuples = [exc] + tc.echoes(225, 2310) + [("SPOILER",), rfc, ("S", -1), rlx, ("ADC", "Z0")] + tc.echoes(225, 2310)
    ops = ops_of(tuples)
    for exact in (False, True):
        enc, records, _ = _functions.compile_sequence(ops, [epg.Jacobian(["magnitude", "T2"])], variables=["T2"])
        enc.deriv_flags |= _lib.DERIV_THROUGH_PLAIN_OPS if exact else 0
        K = enc.capacity()
        assert K == 1024 and enc.peak // _lib.TILED_W == 2, enc.peak
        plan = enc.device_plan(ctx(), K)
        assert _lib.kernel_for(ctx(), plan, K) == "deriv_kernel<16, 1, 1, true>"
        assert _lib.tiled_deriv_info(ctx(), plan, K)["names"] == "tiled_deriv_kernel<8, 32, 1>"
        out = []
        for tiled in (False, True):
            sig = _lib.DeviceBuffer(ctx(), 16 * enc.n_adc * enc.nvox)
            if tiled:
                guarded(lambda: _lib.run_tiled_deriv(ctx(), plan, 0, enc.nvox, None, K, sig.ptr.value, enc.nvox, 0))
            else:
                guarded(lambda: _lib.run(ctx(), plan, 0, plan.n_ops, 0, enc.nvox, None, None, K, sig.ptr.value, enc.nvox, 0))
            out.append(guarded(lambda: sig.download(np.complex128, (len(records), 2, enc.nvox))))
            sig.free()
        assert np.abs(out[0][:, 1]).max() > 0
        assert np.array_equal(out[0], out[1]), float(np.max(np.abs(out[0] - out[1])))


def test_plain_entry_points_still_refuse_derivative_plans():
    ops = ops_of(tc.CASES["t_one"]["tuples"])
    enc, _, _ = _functions.compile_sequence(ops, [epg.Jacobian(["magnitude", "T2"])], variables=["T2"])
    plan = enc.device_plan(ctx())
    for call in (lambda: _lib.tiled_info(ctx(), plan, enc.tiled_capacity()),
                 lambda: _lib.run_tiled(ctx(), plan, 0, enc.nvox, None, enc.tiled_capacity(), 0, enc.nvox, 0)):
        with pytest.raises(_lib.EpgxError, match="derivative states"):
            call()
    plain = _functions.compile_sequence(ops)[0]
    with pytest.raises(_lib.EpgxError, match="derivative states"):
        _lib.tiled_deriv_info(ctx(), plain.device_plan(ctx()), plain.tiled_capacity())


# ------------------------------------------------------------------ (c) voxel slabs
_SLAB_CHILD = """
import sys, numpy as np
sys.path.insert(0, {root!r})
import epgpy_amd as epg
T2 = np.linspace(200, 400, 10)
ops = [epg.T(90, 90)] + [epg.S(1), epg.T(140, 0, order1=True), epg.S(1), epg.E(1, 900, T2, order1=True), epg.ADC] * 530
np.save({out!r}, epg.simulate(ops, probe=epg.Jacobian(["magnitude", "T2", "alpha"]), mode="resident"))
"""


def test_slabs_give_the_same_bits(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = {}
    for name, env in (("one", {}), ("slabs", {"EPGX_SLAB_VOXELS": "4"})):
        out = str(tmp_path / f"{name}.npy")
        code = _SLAB_CHILD.format(root=root, out=out)
        guarded(lambda: subprocess.run([sys.executable, "-c", code], check=True, timeout=300, env={**os.environ, **env}))
        res[name] = np.load(out)
    assert res["one"].shape == (530, 10, 3) and np.abs(res["one"][-1]).min() > 0
    assert np.array_equal(res["one"], res["slabs"])


# ------------------------------------------------------------------ (d) the reference's own numbers
def _golden_generator():
    import importlib.util
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "make_golden_tiled_jacobian.py")
    spec = importlib.util.spec_from_file_location("make_golden_tiled_jacobian", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)      # (the module imports the reference only when run as a program)
    return mod


def test_g23_tiled_jacobian(golden):
    g = golden("g23_tiled_jacobian")
    gen = _golden_generator()
    inputs = gen.inputs()
    for key in g.files:                  # the stored parameters are the generator's
        if key in inputs:
            assert np.array_equal(g[key], inputs[key]), key
    seq = gen.sequence(epg, inputs)
    got = guarded(lambda: epg.simulate(seq, probe=epg.Jacobian(gen.VARIABLES), mode="resident"))
    want = g["jacobian"]
    assert got.shape == want.shape == (530, 3, 3)
    err = float(np.max(np.abs(got - want)))
    assert err <= 1e-11 * max(1.0, float(np.max(np.abs(want)))), err      # (the bound of the g16 / g18 tests)


# ------------------------------------------------------------------ (e) on request only
def test_auto_mode_still_raises():
    ops = ops_of(tc.CASES["t_one"]["tuples"])
    with pytest.raises(NotImplementedError, match="mode='resident'"):
        epg.simulate(ops, probe=epg.Jacobian(["magnitude", "T2"]))
    with pytest.raises(NotImplementedError):          # Hessians above the capacity keep their error
        epg.simulate(ops, probe=epg.Hessian(["magnitude", "T2"], ["T2"]), mode="resident")

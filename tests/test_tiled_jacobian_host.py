"""CPU: Jacobians beyond 1024 orders on the tiled path -- which calls simulate() sends there (on request only:
mode="resident" written out), the float64 floors of the device cases (tests/tiled_jacobian_cases.py) and what keeps their
late echoes sensitive to the upper tiles, and the schedule of a derivative plan (tests/host/tiled_deriv_check.cpp against
the planner that ships).  No GPU needed."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import epgpy_amd as epg
from epgpy_amd import _lib, functions
from oracle import epg_numpy as onp
from tests import tiled_jacobian_cases as tc
from tests.jacobian_recurrence import jacobian_recurrence, grid_of, column_errors

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "epgpy_amd", "csrc")


# ------------------------------------------------------------------ routing
class _Tiled(Exception):
    pass


def _route(monkeypatch, seq, **kw):
    """simulate() up to its choice of path (no device is touched before it): 'tiled', or the exception raised"""
    def tiled(*args, **kwargs):
        raise _Tiled()

    monkeypatch.setattr(functions, "_simulate_jacobian_tiled", tiled)
    monkeypatch.setattr(_lib, "default_device", lambda: 0)
    try:
        epg.simulate(seq, **kw)
    except _Tiled:
        return "tiled"
    except NotImplementedError as exc:
        return f"NotImplementedError: {exc}"
    except Exception as exc:   # pragma: no cover - reached a device call: not the tiled path
        return type(exc).__name__
    return "ran"


T1, T2 = np.array([800.0, 1200.0]), np.array([60.0, 90.0])


def jac_train(shift=None, extra=()):
    return [epg.T(90, 90)] + [shift or epg.S(1), epg.T(30, 0), epg.E(5, 1000, T2, order1=True), *extra, epg.ADC] * 1100


def test_tiled_derivative_path_is_taken_on_request(monkeypatch):
    jac = epg.Jacobian(["magnitude", "T2"])
    assert _route(monkeypatch, jac_train(), probe=jac, mode="resident") == "tiled"
    auto = _route(monkeypatch, jac_train(), probe=jac)
    assert auto.startswith("NotImplementedError") and "mode='resident'" in auto and "1101 phase states" in auto
    assert _route(monkeypatch, jac_train(), probe=jac, mode="auto") == auto
    assert _route(monkeypatch, jac_train(), probe=jac, mode="stream").startswith("NotImplementedError")
    assert _route(monkeypatch, jac_train(), probe=jac, mode="resident", ngpu=2).startswith("NotImplementedError")
    # below the wall nothing changes: the in-register path (which reaches for the device: not "tiled", not NotImplementedError)
    short = [epg.T(90, 90)] + [epg.S(1), epg.E(5, 1000, T2, order1=True), epg.ADC] * 100
    assert not _route(monkeypatch, short, probe=jac, mode="resident").startswith(("tiled", "NotImplementedError"))


def test_what_the_tiled_derivative_path_refuses(monkeypatch):
    jac = epg.Jacobian(["magnitude", "T2"])
    kw = dict(probe=jac, mode="resident")
    assert _route(monkeypatch, jac_train(shift=epg.S([1, 0])), **kw).startswith("NotImplementedError")          # n-D shifts
    assert _route(monkeypatch, jac_train(extra=[epg.D(5, 1e-3)]), **kw).startswith("NotImplementedError")       # diffusion
    ex = [epg.T(90, 90), epg.X(5, 0.01, T1=[800, 1000], T2=[40, 80], axis=0), epg.ADC] + \
         [epg.S(1), epg.T(30, 0), epg.E(5, 1000, 80.0, order1=True)] * 1100 + [epg.ADC]
    assert _route(monkeypatch, ex, **kw).startswith(("NotImplementedError", "ValueError"))                      # exchange
    # (a Hessian above the capacity raises after it has opened the device: tests/test_gpu_tiled_jacobian.py)
    hess = functions.compile_sequence(jac_train(), variables=["T2", "T2:T2"], hessian=("T2", "T2"), fuse=False, collapse=False)[0]
    assert hess.deriv_flags & _lib.DERIV_SECOND and not hess.tiled_ok(derivatives=True)


def test_predicates():
    enc = functions.compile_sequence(jac_train(), variables=["T2"])[0]
    assert not enc.tiled_ok()                       # the zero-argument form: no derivative states
    assert enc.tiled_ok(derivatives=True)
    assert not functions.compile_sequence(jac_train())[0].tiled_ok(derivatives=True)       # no variables: the plain entry
    assert functions.compile_sequence(jac_train())[0].tiled_ok()
    many = functions.compile_sequence([epg.T(30, 0, order1=True)] + jac_train(), variables=["T2", "alpha", "phi"])[0]
    assert _lib.TILED_DERIV_V == 2 and not many.tiled_ok(derivatives=True)                # more than a launch carries
    nd = functions.compile_sequence(jac_train(shift=epg.S([1, 1])), variables=["T2"])[0]
    assert not nd.tiled_ok(derivatives=True)
    dif = functions.compile_sequence(jac_train(extra=[epg.D(5, 1e-3)]), variables=["T2"])[0]
    assert not dif.tiled_ok(derivatives=True)
    assert (_lib.TILED_M, _lib.TILED_H, _lib.TILED_W) == (8, 32, 448)


def test_entry_points_are_declared_bound_and_documented():
    root = os.path.join(HERE, "..")
    header = open(os.path.join(root, "include", "epgx.h")).read()
    doc = open(os.path.join(root, "INTEGRATION.md")).read()
    for name in ("epgx_run_tiled_deriv", "epgx_tiled_deriv_info"):
        assert name in header and name in _lib.SYMBOLS and name in doc
    assert len(_lib.SYMBOLS["epgx_run_tiled_deriv"][1]) == len(_lib.SYMBOLS["epgx_run_tiled"][1])
    assert len(_lib.SYMBOLS["epgx_tiled_deriv_info"][1]) == len(_lib.SYMBOLS["epgx_tiled_info"][1])
    assert _lib.ABI_VERSION == 11


# ------------------------------------------------------------------ floors
_MEASURED = {}


def measured(name):
    """(float64 floor, per probe the extended-precision records) of a case, once per module"""
    if name not in _MEASURED:
        c = tc.CASES[name]
        tuples = tc.full_tuples(c)
        kw = dict(max_nstate=c["cap"], through_plain=c["exact"], shape=grid_of(tc.plain(c["tuples"])))
        floor, wants = 0.0, {}
        for probe in c["probes"]:
            want = jacobian_recurrence(tuples, c["variables"], probe=probe, **kw)
            got = onp.simulate_jacobian(tuples, ["magnitude"] + c["variables"], probe=probe, **kw)
            floor = max(floor, max(column_errors(got, want, zero_atol=1e-17)))
            wants[probe] = want
        _MEASURED[name] = (floor, wants)
    return _MEASURED[name]


@pytest.mark.parametrize("name", list(tc.CASES))
def test_floors_and_late_echoes(name):
    floor, wants = measured(name)
    print(name, "float64 floor", floor)
    assert floor <= tc.FLOORS[name], (name, floor)
    assert 0 < 16 * tc.FLOORS[name] <= 1e-11, name
    c = tc.CASES[name]
    for probe, want in wants.items():
        assert want.shape[0] >= tc.LATE + 30 and want.shape[1] % 4 != 0
        for v in range(want.shape[-1]):
            col = np.abs(want[..., v])
            assert col[tc.LATE:].max() >= 1e-3 * col.max(), (name, probe, v, float(col[tc.LATE:].max() / col.max()))
    # every case populates more than 1024 orders: simulate() cannot run it in registers
    enc = functions.compile_sequence(tc_ops(c), variables=c["variables"][:1], options={"max_nstate": c["cap"]} if c["cap"] else {},
                                     nstate0=604 if c["head"] else 0, dense_start=bool(c["head"]))[0]
    assert enc.peak + 1 > _lib.MAX_DERIV_K and enc.peak // _lib.TILED_W >= 2, enc.peak


def tc_ops(c):
    from tests.jacobian_cases import ops_of
    return ops_of(c["tuples"])


def test_floor_table_names_every_case():
    assert set(tc.FLOORS) == set(tc.CASES)


# ------------------------------------------------------------------ the schedule of a derivative plan
def test_tiled_deriv_check(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "tiled_deriv_check")
    subprocess.check_call([cxx, "-O1", "-std=c++17", "-Wall", "-Wextra", "-o", exe,
                           os.path.join(HERE, "host", "tiled_deriv_check.cpp"), os.path.join(CSRC, "epgx_planner.cpp")])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(run.stdout[-4000:])
    assert run.returncode == 0, run.stdout[-2000:]
    assert run.stdout.rstrip().endswith("tiled_deriv_check: all checks passed")

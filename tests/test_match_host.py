"""CPU: the C boundary of epgx_signal_norms / epgx_signal_match, the argument checks of epgpy_amd.match that need no GPU, and the
condition on the inputs of tests/test_gpu_match.py: at least 90 % of the voxels of every case are decisive under the
extended-precision yardstick alone (tests/match_cases.py), so that the tolerance rule cannot hide a wrong argmax."""
import os
import re

import numpy as np
import pytest

from epgpy_amd import match, functions, _lib, _build
from tests import match_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_boundary_agrees():
    """include/epgx.h, _lib.py, INTEGRATION.md and the built library: both entry points, still ABI 11"""
    header = open(os.path.join(ROOT, "include", "epgx.h")).read()
    assert "#define EPGX_ABI_VERSION 11" in header and _lib.ABI_VERSION == 11
    for name, nargs in (("epgx_signal_norms", 6), ("epgx_signal_match", 13)):
        proto = re.search(rf"int {name}\(([^)]*)\)", header).group(1)
        assert len(proto.split(",")) == len(_lib.SYMBOLS[name][1]) == nargs, name
    lib = _lib.load()
    assert lib.epgx_abi_version() == 11 and hasattr(lib, "epgx_signal_norms") and hasattr(lib, "epgx_signal_match")
    assert any(src == "epgx_match.hip" for _, src, _ in _build.UNITS)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "epgx_signal_norms" in doc and "epgx_signal_match" in doc
    assert callable(_lib.signal_norms) and callable(_lib.signal_match)
    import inspect
    assert inspect.signature(_lib.signal_match).parameters["nsplit"].default == 0


def test_raw_entries_validate_before_any_device_work():
    """NULL arguments are refused without a context: EPGX_ERR_INVALID and a message"""
    lib = _lib.load()
    assert lib.epgx_signal_norms(None, None, 0, 1, 1, None) == -1
    assert b"epgx_signal_norms" in lib.epgx_last_error()
    assert lib.epgx_signal_match(None, None, 0, None, 1, None, 0, 1, 0, 0, None, None, None) == -1
    assert b"epgx_signal_match" in lib.epgx_last_error()


def test_split_bounds():
    """the ranges of the header's rule cover the atoms once, in order, sizes differing by at most one"""
    for natoms, nsplit in ((257, 3), (257, 2), (33, 33), (17, 1), (16, 5), (1000000, 7)):
        b = _lib.match_split_bounds(natoms, nsplit)
        assert b == mc.split_bounds(natoms, nsplit)
        assert b[0][0] == 0 and b[-1][1] == natoms and all(x[1] == y[0] for x, y in zip(b, b[1:]))
        sizes = [hi - lo for lo, hi in b]
        assert max(sizes) - min(sizes) <= 1 and sizes == sorted(sizes, reverse=True)


class _Ptr:
    value = 1 << 20


class _Buf:
    """stands in for a DeviceBuffer: the checks under test raise before anything touches it"""
    class ctx:
        device = 0
    ptr = _Ptr()


def test_argument_errors_before_the_device():
    whole = functions.DeviceSignal(_Buf(), 6, (5, 7), 0, 1)
    part = functions.DeviceSignal(_Buf(), 6, (5, 7), 0, 1, vox0=0, count=20)
    sharded = functions.ShardedDeviceSignal([part], (5, 7))
    sig = np.zeros((6, 3))
    for bad in (sharded, part):
        with pytest.raises(NotImplementedError, match="dictionary"):
            match.match(bad, sig)
        with pytest.raises(NotImplementedError, match="dictionary"):
            match.Dictionary(bad)
        with pytest.raises(NotImplementedError, match="signals"):
            match.match(whole, bad)
    with pytest.raises(ValueError, match="records"):                 # nrec mismatch: handle and host dictionaries
        match.match(whole, np.zeros((5, 3)))
    with pytest.raises(ValueError, match="records"):
        match.match(np.zeros((6, 4, 4)), np.zeros((5, 3)))
    with pytest.raises(ValueError, match="dictionary"):               # wrong ndim: no grid axis
        match.Dictionary(np.zeros(6))
    with pytest.raises(ValueError, match="dictionary"):
        match.match(np.zeros(6), sig)
    with pytest.raises(ValueError, match="signals"):                  # wrong ndim: no record axis
        match.match(whole, np.float64(1.0))
    with pytest.raises(ValueError, match="signals"):
        match.match(whole, np.array(["a", "b", "c", "d", "e", "f"]))


def test_jacobian_view_is_the_probed_state_row():
    jac = functions.DeviceJacobian(_Buf(), 6, (5, 7), 2, 3, 1, [0, 2], ["magnitude", "T2"])
    view = match._signal_handle(jac, "dictionary")
    assert view.ptr == jac.ptr and view.row_stride == jac.record_stride and view.shape == (6, 5, 7) and view.whole


def test_unravel():
    res = match.MatchResult(np.array([[3, -1], [34, 0]]), None, None, (5, 7))
    i, j = res.unravel()
    assert (i == [[0, -1], [4, 0]]).all() and (j == [[3, -1], [6, 0]]).all()


@pytest.fixture(scope="module")
def cases():
    return mc.cases()


def test_every_gpu_case_is_decisive(cases):
    for name, (D, S) in cases.items():
        y = mc.Yardstick(D, S)
        share = y.decisive.mean()
        assert share >= 0.9, (name, float(share))


def test_yardstick_accepts_float64_and_rejects_a_wrong_atom(cases):
    """the plain float64 formula passes the yardstick; an index off by one, a scale off by 1e-12 relative do not"""
    D, S = cases["gauss_33_67_37"]
    y = mc.Yardstick(D, S)
    n = (np.abs(D) ** 2).sum(0)
    c = np.conj(D).T @ S
    q = np.abs(c) ** 2 / n[:, None]
    idx = np.argmax(q, axis=0)
    m = np.arange(S.shape[1])
    scale = c[idx, m] / n[idx]
    score = np.minimum(np.sqrt(q[idx, m] / (np.abs(S) ** 2).sum(0)), 1.0)
    y.check(idx, scale, score)
    with pytest.raises(AssertionError):
        y.check((idx + 1) % 33, scale, score)
    with pytest.raises(AssertionError):
        y.check(idx, scale * (1 + 1e-12), score)
    with pytest.raises(AssertionError):
        y.check(idx, scale, score * (1 - 1e-12))


def test_tie_and_invalid_cases_are_what_they_say():
    D, S, expect = mc.tie_case()
    y = mc.Yardstick(D, S)
    assert (y.amax == expect).all() and y.decisive.all()
    D, S, _ = mc.invalid_case()
    y = mc.Yardstick(D, S)
    assert list(np.flatnonzero(~y.valid)) == [3, 8, 16] and y.energy[4] == 0

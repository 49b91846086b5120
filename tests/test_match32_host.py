"""CPU: the C boundary of epgx_signal_norms_c64 / epgx_signal_match_c64 (and epgx_signal_narrow, which they build on), the argument
checks of the complex64 route of epgpy_amd.match that need no GPU, and the condition on the inputs of tests/test_gpu_match32.py:
at least 90 % of the voxels of every case are decisive under the float32 yardstick alone (tests/match32_cases.py), so that the
tolerance rule cannot hide a wrong argmax."""
import os
import re

import numpy as np
import pytest

from epgpy_amd import match, functions, _lib, _build
from tests import match32_cases as m32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROTOTYPES = (("epgx_signal_narrow", 7), ("epgx_signal_norms_c64", 6), ("epgx_signal_match_c64", 13))


def test_boundary_agrees():
    """include/epgx.h, _lib.py, INTEGRATION.md and the built library: the three entry points, still ABI 11, the new unit"""
    header = open(os.path.join(ROOT, "include", "epgx.h")).read()
    assert "#define EPGX_ABI_VERSION 11" in header and _lib.ABI_VERSION == 11
    lib = _lib.load()
    assert lib.epgx_abi_version() == 11
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name, nargs in PROTOTYPES:
        found = re.findall(rf"int {name}\(([^)]*)\)", header)
        assert len(found) == 1, name
        assert len(found[0].split(",")) == len(_lib.SYMBOLS[name][1]) == nargs, name
        assert hasattr(lib, name) and name in doc, name
    # the complex64 calls take what the complex128 calls take, in the same order
    assert _lib.SYMBOLS["epgx_signal_norms_c64"] == _lib.SYMBOLS["epgx_signal_norms"]
    assert _lib.SYMBOLS["epgx_signal_match_c64"] == _lib.SYMBOLS["epgx_signal_match"]
    assert any(src == "epgx_match32.hip" for _, src, _ in _build.UNITS)
    assert "epgx_match32.h" in _build.include_closure("epgx_signal.hip")
    import inspect
    assert inspect.signature(_lib.signal_match).parameters["c64"].default is False
    assert inspect.signature(_lib.signal_norms).parameters["c64"].default is False


def test_raw_entries_validate_before_any_device_work():
    """NULL arguments are refused without a context: EPGX_ERR_INVALID and a message"""
    lib = _lib.load()
    assert lib.epgx_signal_narrow(None, None, 0, None, 0, 1, 1) == -1
    assert b"epgx_signal_narrow" in lib.epgx_last_error()
    assert lib.epgx_signal_norms_c64(None, None, 0, 1, 1, None) == -1
    assert b"epgx_signal_norms_c64" in lib.epgx_last_error()
    assert lib.epgx_signal_match_c64(None, None, 0, None, 1, None, 0, 1, 0, 0, None, None, None) == -1
    assert b"epgx_signal_match_c64" in lib.epgx_last_error()


class _Ptr:
    value = 1 << 20


class _Buf:
    """stands in for a DeviceBuffer: the checks under test raise before anything touches it"""
    class ctx:
        device = 0
    ptr = _Ptr()


def _c64_dictionary(nrec=6, grid=(5, 7)):
    """a complex64 `Dictionary` without a device: what the argument checks look at, nothing else"""
    dic = object.__new__(match.Dictionary)
    dic.dtype, dic.nrec, dic.grid, dic.natoms, dic.basis = np.dtype(np.complex64), nrec, grid, int(np.prod(grid)), None
    return dic


def test_argument_errors_before_the_device():
    D = np.zeros((6, 5, 7))
    for bad in (np.float32, np.float64, "int32", np.complex256 if hasattr(np, "complex256") else "S4", object):
        with pytest.raises(ValueError, match="dtype"):
            match.Dictionary(D, dtype=bad)
        with pytest.raises(ValueError, match="dtype"):
            match.compress(D, rank=2, dtype=bad)
    whole = functions.DeviceSignal(_Buf(), 6, (5, 7), 0, 1)
    part = functions.DeviceSignal(_Buf(), 6, (5, 7), 0, 1, vox0=0, count=20)
    sharded = functions.ShardedDeviceSignal([part], (5, 7))
    for bad in (sharded, part):                                        # what they raise without a dtype
        with pytest.raises(NotImplementedError, match="dictionary"):
            match.Dictionary(bad, dtype=np.complex64)
        with pytest.raises(NotImplementedError, match="dictionary"):
            match.compress(bad, rank=2, dtype=np.complex64)
    with pytest.raises(ValueError, match="dictionary"):                # wrong ndim: no grid axis
        match.Dictionary(np.zeros(6), dtype=np.complex64)
    dic = _c64_dictionary()
    with pytest.raises(NotImplementedError, match="complex64"):        # no single-precision Gram matrix
        match.compress(dic, rank=2)
    with pytest.raises(NotImplementedError, match="complex64"):
        match.compress(dic, rank=2, dtype=np.complex64)
    with pytest.raises(NotImplementedError, match="widen"):
        dic.astype(np.complex128)
    with pytest.raises(ValueError, match="dtype"):
        dic.astype(np.float32)
    assert dic.astype(np.complex64) is dic and dic.astype("complex64") is dic
    with pytest.raises(NotImplementedError, match="download"):
        dic.records
    with pytest.raises(ValueError, match="records"):                   # nrec mismatch against a complex64 dictionary
        match.match(dic, np.zeros((5, 3)))
    with pytest.raises(NotImplementedError, match="signals"):
        match.match(dic, part)
    assert whole.whole


def test_host_rounding_is_astype():
    """the host route of `Dictionary(array, dtype=complex64)`: `_Records.narrowed` is `astype(np.complex64)`, bit for bit, also
    for real input and for complex64 input (which it leaves as it is)"""
    vals = m32.narrow_values((5, 257))
    rec = match._Records(vals, "dictionary").narrowed()
    assert rec.dtype == np.complex64 and rec._host.dtype == np.complex64 and rec._host.shape == (5, 257) and rec.row_stride == 257
    with np.errstate(over="ignore", invalid="ignore"):
        want = vals.astype(np.complex64)
    assert rec._host.tobytes() == want.tobytes()
    assert np.isinf(want.real).sum() >= 6 and (np.abs(want.real[np.isfinite(want.real)]) < 2.0 ** -126).any()
    again = match._Records(want, "dictionary").narrowed()
    assert again._host.tobytes() == want.tobytes()
    real = match._Records(vals.real[:, :20], "signals").narrowed()
    with np.errstate(over="ignore", invalid="ignore"):
        assert real._host.tobytes() == vals.real[:, :20].astype(np.complex64).tobytes()


@pytest.fixture(scope="module")
def cases():
    return m32.cases()


def test_every_gpu_case_is_decisive(cases):
    assert m32.CHUNK == 64 and m32.KSTEP == 4
    header = open(os.path.join(ROOT, "epgpy_amd", "csrc", "epgx_signal_limits.h")).read()
    assert re.search(r"MATCH32_CHUNK\s*=\s*64\b", header)
    names = set(cases)
    for nrec in (63, 64, 65, 129, 6):
        assert f"gauss_33_17_{nrec}" in names
    assert "decay_257_67_37" not in names and "decay_33_17_5" not in names
    for name, (D, S) in cases.items():
        y = m32.Yardstick32(D, S)
        share = y.decisive.mean()
        print(name, "decisive:", float(share))
        assert share >= 0.9, (name, float(share))


def test_close_case_has_no_decisive_voxel():
    y = m32.Yardstick32(*m32.close_case())
    assert not y.decisive.any()


def test_yardstick_accepts_float32_accumulation_and_rejects_a_wrong_atom(cases):
    """a float32 evaluation (numpy complex64 matmul on the rounded operands, norms in float64) passes; an index off by one, a
    scale or score off by 1e-4 relative, norms off by 1e-12 relative or summed in float32 do not"""
    D, S = cases["gauss_33_67_37"]
    y = m32.Yardstick32(D, S)
    D32, S32 = m32.fl32(D), m32.fl32(S)
    n = (np.abs(D32.astype(np.complex128)) ** 2).sum(0)
    c = (np.conj(D32).T @ S32).astype(np.complex128)            # accumulated in float32
    q = np.abs(c) ** 2 / n[:, None]
    idx = np.argmax(q, axis=0)
    m = np.arange(S.shape[1])
    scale = c[idx, m] / n[idx]
    score = np.minimum(np.sqrt(q[idx, m] / (np.abs(S32.astype(np.complex128)) ** 2).sum(0)), 1.0)
    y.check(idx, scale, score)
    y.check_norms(n)
    with pytest.raises(AssertionError):
        y.check((idx + 1) % 33, scale, score)
    with pytest.raises(AssertionError):
        y.check(idx, scale * (1 + 1e-4), score)
    with pytest.raises(AssertionError):
        y.check(idx, scale, score * (1 - 1e-4))
    with pytest.raises(AssertionError):
        y.check_norms(n * (1 + 1e-12))
    with pytest.raises(AssertionError):                              # norms summed in float32 miss the float64 bound
        y.check_norms((np.abs(D32) ** 2).sum(0, dtype=np.float32).astype(np.float64))


def test_tie_and_invalid_cases_are_what_they_say():
    from tests import match_cases as mc
    D, S, expect = mc.tie_case()
    y = m32.Yardstick32(D, S)
    assert (y.amax == expect).all() and y.decisive.all()
    D, S, _ = mc.invalid_case()
    y = m32.Yardstick32(D, S)
    assert list(np.flatnonzero(~y.valid)) == [3, 8, 16] and y.energy[4] == 0
    D = D.copy()
    D[0, 5] = 3.5e38                                                 # finite in float64, Inf once rounded
    y = m32.Yardstick32(D, S)
    assert list(np.flatnonzero(~y.valid)) == [3, 5, 8, 16]

"""GPU: epgpy_amd.match (norms_kernel, match_kernel, match_merge_kernel of csrc/epgx_match.hip) against the extended-precision
yardstick of tests/match_cases.py, whose bounds are derived there and not measured.  Shapes sit around the 16 x 16 x 4 MFMA tile,
the 64-voxel workgroup, the 64-atom pass of a workgroup and the 32-record LDS chunk; tests/test_match_host.py shows on the CPU
that at least 90 % of the voxels of every case are decisive, i.e. must return the reference argmax exactly."""
import ctypes

import numpy as np
import pytest

from tests import match_cases as mc

pytestmark = pytest.mark.gpu

CASES = mc.cases()
_YARD = {}


def yard(name):
    if name not in _YARD:
        _YARD[name] = mc.Yardstick(*CASES[name])
    return _YARD[name]


@pytest.fixture(scope="module")
def ctx():
    from epgpy_amd import _lib
    return _lib.get_context()


def padded(ctx, A, pad, lead=0):
    """A [nrec, ncol] in a device buffer with rows of ncol + pad elements, `lead` elements in; padding and lead hold NaN (a
    kernel that read them would show it).  Returns (buffer, address of A[0, 0], row stride)"""
    from epgpy_amd import _lib
    nrec, ncol = A.shape
    host = np.full(lead + nrec * (ncol + pad), np.nan + 1j * np.nan, dtype=np.complex128)
    host[lead:].reshape(nrec, ncol + pad)[:, :ncol] = A
    buf = _lib.DeviceBuffer(ctx, host.nbytes)
    buf.upload(host)
    return buf, buf.ptr.value + 16 * lead, ncol + pad


def raw_match(ctx, D, S, nsplit=0, dpad=0, spad=0, lead=0):
    """through _lib.signal_norms / _lib.signal_match on buffers of this test's making"""
    from epgpy_amd import _lib
    dbuf, dptr, dstride = padded(ctx, D, dpad, lead)
    sbuf, sptr, sstride = padded(ctx, S, spad, lead)
    norms = _lib.signal_norms(ctx, dptr, dstride, D.shape[0], D.shape[1])
    try:
        return _lib.signal_match(ctx, dptr, dstride, norms.ptr.value, D.shape[1], sptr, sstride, D.shape[0], S.shape[1], nsplit=nsplit)
    finally:
        for b in (dbuf, sbuf, norms):
            b.free()


def same_bits(got, want):
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes()


@pytest.mark.parametrize("name", sorted(CASES))
def test_case_against_yardstick(name):
    """every shape, the correlated dictionaries, the 1000-record case, ties and invalid atoms through match.match on host arrays"""
    from epgpy_amd import match
    D, S = CASES[name]
    res = match.match(D[:, :, None], S)               # (a grid with a trailing axis of one: the flat index is unchanged)
    assert res.index.shape == res.scale.shape == res.score.shape == (S.shape[1],)
    worst = yard(name).check(res.index, res.scale, res.score, what=name)
    print(name, "largest share of the bounds used:", worst)


def test_norms(ctx):
    from epgpy_amd import match
    D, _ = CASES["gauss_257_67_5"]
    dic = match.Dictionary(D)
    assert dic.grid == (257,) and dic.natoms == 257 and dic.nrec == 5
    y = yard("gauss_257_67_5")
    got = dic.norms
    assert got.shape == (257,) and got.dtype == np.float64
    assert np.all(np.abs(got.astype(np.longdouble) - y.n) <= y.g * y.n)


@pytest.mark.parametrize("name", ["gauss_257_67_5", "gauss_33_67_37", "gauss_17_17_5", "tie", "gauss_33_17_1000"])
def test_forced_splits_agree_bit_for_bit(ctx, name):
    """nsplit = 1, 2, 3 and natoms through _lib.signal_match: the true atoms lie on both sides of every range boundary
    (match_cases.placements); all equal the library's own choice bit for bit, and that one passes the yardstick"""
    D, S = CASES[name]
    auto = raw_match(ctx, D, S)
    yard(name).check(*auto, what=name)
    for nsplit in (1, 2, 3, D.shape[1]):
        same_bits(raw_match(ctx, D, S, nsplit=nsplit), auto)


def test_ties_return_the_lowest_index(ctx):
    D, S, expect = mc.tie_case()
    for nsplit in (0, 1, 2, 3, 33):
        index, _, _ = raw_match(ctx, D, S, nsplit=nsplit)
        assert (index == expect).all(), (nsplit, index, expect)


def test_invalid_atoms(ctx):
    from epgpy_amd import match
    D, S, _ = mc.invalid_case()
    for nsplit in (0, 1, 3, 17):
        index, scale, score = raw_match(ctx, D, S, nsplit=nsplit)
        assert not np.isin(index, [3, 8, 16]).any() and (index >= 0).all()
        assert score[4] == 0.0 and scale[4] == 0.0 and np.isfinite(score).all() and np.isfinite(scale).all()
        yard("invalid").check(index, scale, score)
    none = np.zeros((5, 17), dtype=np.complex128)
    none[1, ::2] = np.nan
    res = match.match(none, S)
    assert (res.index == -1).all() and (res.scale == 0).all() and (res.score == 0).all()
    assert all((ax == -1).all() for ax in res.unravel())


def test_strides(ctx):
    """row strides beyond the columns, buffers that do not start at the records: through the raw entry and through handles (a
    dictionary that is the second of three probes of its buffer, signals that are the first of two)"""
    from epgpy_amd import match, functions, _lib
    name = "gauss_33_67_37"
    D, S = CASES[name]
    dense = raw_match(ctx, D, S)
    yard(name).check(*dense, what=name)
    same_bits(raw_match(ctx, D, S, dpad=3, spad=5, lead=7), dense)

    nrec = D.shape[0]
    dhost = np.full((nrec, 3, 33), np.nan + 0j)
    dhost[:, 1] = D
    shost = np.full((nrec, 2, 67), np.nan + 0j)
    shost[:, 0] = S
    dbuf, sbuf = _lib.DeviceBuffer(ctx, dhost.nbytes), _lib.DeviceBuffer(ctx, shost.nbytes)
    dbuf.upload(dhost)
    sbuf.upload(shost)
    dsig = functions.DeviceSignal(dbuf, 3 * nrec, (3, 11), 1, 3)
    ssig = functions.DeviceSignal(sbuf, 2 * nrec, (67,), 0, 2)
    assert dsig.row_stride == 99 and ssig.row_stride == 134 and dsig.shape == (nrec, 3, 11)
    dic = match.Dictionary(dsig)
    assert dic.grid == (3, 11) and dic.natoms == 33 and dic.nrec == nrec
    res = match.match(dic, ssig)
    same_bits((res.index, res.scale, res.score), dense)
    again = match.match(dsig, S.reshape(nrec, 67))
    same_bits((again.index, again.scale, again.score), dense)
    ax = res.unravel()
    want = np.unravel_index(dense[0], (3, 11))
    assert all((a == w).all() for a, w in zip(ax, want))


def test_a_voxel_does_not_depend_on_the_others(ctx):
    from epgpy_amd import match
    for name in ("gauss_33_67_37", "decay_257_67_37", "gauss_257_67_5"):
        D, S = CASES[name]
        dic = match.Dictionary(D)
        full = match.match(dic, S)
        part = match.match(dic, S[:, 5:22])
        same_bits((part.index, part.scale, part.score), (full.index[5:22], full.scale[5:22], full.score[5:22]))
        one = match.match(dic, S[:, 40])
        same_bits((one.index.reshape(1), one.scale.reshape(1), one.score.reshape(1)),
                  (full.index[40:41], full.scale[40:41], full.score[40:41]))
        assert one.index.shape == ()


def test_signal_shapes_and_real_signals(ctx):
    from epgpy_amd import match
    D, S = CASES["gauss_17_17_5"]
    real = np.ascontiguousarray(S.real[:, :12]).reshape(5, 3, 4)
    res = match.match(D, real)
    assert res.index.shape == (3, 4) and res.scale.dtype == np.complex128
    mc.Yardstick(D, real.reshape(5, 12).astype(np.complex128)).check(res.index, res.scale, res.score)
    empty = match.match(D, np.zeros((5, 0)))
    assert empty.index.shape == (0,) and empty.score.shape == (0,)


def test_end_to_end_from_the_simulator(ctx):
    """8 x 9 (T1, T2) multi-spin-echo dictionary of 6 echoes left on the device, as a DeviceSignal and as a DeviceJacobian;
    signals simulated at off-grid parameters"""
    from epgpy_amd import epg, match, functions
    T1 = np.geomspace(400.0, 2000.0, 8)[:, None]
    T2 = np.geomspace(30.0, 200.0, 9)[None, :]

    def train(t1, t2, **kw):
        rlx = epg.E(5.0, t1, t2, **kw)
        return [epg.T(90, 90)] + [epg.S(1), rlx, epg.T(150, 0), epg.S(1), rlx, epg.ADC] * 6

    handle = epg.simulate(train(T1, T2), out="device")
    if isinstance(handle, (tuple, list)):
        handle = handle[0]
    assert isinstance(handle, functions.DeviceSignal) and handle.shape == (6, 8, 9)
    rng = np.random.default_rng(21)
    t1 = rng.uniform(450.0, 1900.0, 11)
    t2 = rng.uniform(35.0, 190.0, 11)
    pd = (0.5 + rng.random(11)) * np.exp(2j * np.pi * rng.random(11))
    S = np.asarray(epg.simulate(train(t1, t2))).reshape(6, 11) * pd

    D = np.asarray(handle)
    res = match.match(handle, S)
    y = mc.Yardstick(D.reshape(6, 72), S)
    y.check(res.index, res.scale, res.score, what="mse")
    i1, i2 = res.unravel()
    w1, w2 = np.unravel_index(res.index, (8, 9))
    assert (i1 == w1).all() and (i2 == w2).all()
    host = match.match(D, S)
    same_bits((host.index, host.scale, host.score), (res.index, res.scale, res.score))

    jac = epg.simulate(train(T1, T2, order1=["T2"]), probe=epg.Jacobian(["magnitude", "T2"]), out="device")
    if isinstance(jac, (tuple, list)):
        jac = jac[0]
    assert isinstance(jac, functions.DeviceJacobian)
    Dj = np.asarray(match._signal_handle(jac, "dictionary"))
    resj = match.match(jac, S)
    assert resj.grid == (8, 9)
    mc.Yardstick(Dj.reshape(6, 72), S).check(resj.index, resj.scale, resj.score, what="mse jacobian")


def test_freed_buffer_gives_the_library_error(ctx):
    from epgpy_amd import match, functions, _lib
    D, S = CASES["gauss_17_17_5"]
    buf = _lib.DeviceBuffer(ctx, D.nbytes)
    buf.upload(D)
    sig = functions.DeviceSignal(buf, 5, (17,), 0, 1)
    dic = match.Dictionary(sig)
    buf.free()
    with pytest.raises(_lib.EpgxError):
        match.match(dic, S)
    with pytest.raises(_lib.EpgxError):
        match.Dictionary(sig)


def test_entry_point_errors(ctx):
    """every EPGX_ERR_INVALID condition of include/epgx.h through raw calls: -1, a message, nothing launched"""
    from epgpy_amd import _lib
    lib = ctx.lib
    natoms, nmeas, nrec = 17, 15, 5
    D, S = CASES["gauss_17_17_5"]
    S = np.ascontiguousarray(S[:, :nmeas])
    dbuf, sbuf = _lib.DeviceBuffer(ctx, D.nbytes), _lib.DeviceBuffer(ctx, S.nbytes)
    dbuf.upload(D)
    sbuf.upload(S)
    nbuf = _lib.DeviceBuffer(ctx, 8 * natoms, itemsize=8)
    out = _lib.DeviceBuffer(ctx, 32 * nmeas, itemsize=8)
    d, s, n, o = dbuf.ptr.value, sbuf.ptr.value, nbuf.ptr.value, out.ptr.value
    P = ctypes.c_void_p

    def norms(dict_=d, stride=natoms, nrec_=nrec, natoms_=natoms, out_=n):
        return lib.epgx_signal_norms(ctx.handle, P(dict_) if dict_ else None, stride, nrec_, natoms_, P(out_) if out_ else None)

    def run(dict_=d, dstride=natoms, norms_=n, natoms_=natoms, sig=s, sstride=nmeas, nrec_=nrec, nmeas_=nmeas, nsplit=0,
            index=o + 16 * nmeas, scale=o, score=o + 24 * nmeas):
        p = lambda v: P(v) if v else None      # noqa: E731
        return lib.epgx_signal_match(ctx.handle, p(dict_), dstride, p(norms_), natoms_, p(sig), sstride, nrec_, nmeas_, nsplit,
                                     p(index), p(scale), p(score))

    assert norms() == 0 and run() == 0
    ctx.synchronize()
    good = out.download(np.float64, (4 * nmeas,)).copy()
    big = 1 << 62
    bad_norms = [dict(dict_=0), dict(out_=0), dict(dict_=d + 8), dict(out_=n + 4), dict(nrec_=0), dict(natoms_=0), dict(natoms_=-1),
                 dict(stride=natoms - 1), dict(stride=big, nrec_=2 ** 31 - 1)]
    for kw in bad_norms:
        assert norms(**kw) == -1, kw
        assert b"epgx_signal_norms" in lib.epgx_last_error()
    bad_match = [dict(dict_=0), dict(norms_=0), dict(sig=0), dict(index=0), dict(scale=0), dict(score=0),
                 dict(dict_=d + 8), dict(sig=s + 8), dict(scale=o + 8), dict(norms_=n + 4), dict(index=o + 16 * nmeas + 4),
                 dict(score=o + 24 * nmeas + 4), dict(nrec_=0), dict(nrec_=-3), dict(natoms_=0), dict(nmeas_=-1), dict(nsplit=-1),
                 dict(nsplit=natoms + 1), dict(dstride=natoms - 1), dict(sstride=nmeas - 1), dict(dstride=big, nrec_=2 ** 31 - 1),
                 dict(sstride=big, nrec_=2 ** 31 - 1)]
    for kw in bad_match:
        assert run(**kw) == -1, kw
        assert b"epgx_signal_match" in lib.epgx_last_error()
    assert run(nmeas_=0) == 0 and run(nmeas_=0, sstride=0) == 0          # nothing to do
    assert run(nsplit=natoms) == 0
    ctx.synchronize()
    assert out.download(np.float64, (4 * nmeas,)).tobytes() == good.tobytes()      # the refused calls wrote nothing
    for b in (dbuf, sbuf, nbuf, out):
        b.free()

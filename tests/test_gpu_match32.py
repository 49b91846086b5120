"""GPU: single-precision matching (norms32_kernel, match32_kernel, match32_merge_kernel of csrc/epgx_match32.hip; narrow_kernel
through epgx_signal_narrow) against the extended-precision yardstick of tests/match32_cases.py on the ROUNDED operands, whose
bounds are derived there from the float32 unit roundoff and not measured.  Shapes sit around the 16 x 16 x 4 MFMA tile, the
64-voxel workgroup, the 64-atom pass of a workgroup and the 64-record LDS chunk; tests/test_match32_host.py shows on the CPU that
at least 90 % of the voxels of every case are decisive, i.e. must return the reference argmax exactly."""
import numpy as np
import pytest

from tests import match_cases as mc
from tests import match32_cases as m32
from tests import compress_cases as cc

pytestmark = pytest.mark.gpu

C64 = np.complex64
CASES = m32.cases()
_YARD = {}


def yard(name):
    if name not in _YARD:
        _YARD[name] = m32.Yardstick32(*CASES[name])
    return _YARD[name]


@pytest.fixture(scope="module")
def ctx():
    from epgpy_amd import _lib
    return _lib.get_context()


def padded(ctx, A, pad, lead=0):
    """A [nrec, ncol] (complex64 or complex128) in a device buffer with rows of ncol + pad elements, `lead` elements in; padding
    and lead hold NaN (a kernel that read them would show it).  Returns (buffer, address of A[0, 0], row stride)"""
    from epgpy_amd import _lib
    nrec, ncol = A.shape
    host = np.full(lead + nrec * (ncol + pad), np.nan + 1j * np.nan, dtype=A.dtype)
    host[lead:].reshape(nrec, ncol + pad)[:, :ncol] = A
    buf = _lib.DeviceBuffer(ctx, max(host.nbytes, 16))
    buf.upload(host)
    return buf, buf.ptr.value + A.dtype.itemsize * lead, ncol + pad


def raw_match(ctx, D, S, nsplit=0, dpad=0, spad=0, lead=0):
    """through _lib.signal_norms / _lib.signal_match (c64) on complex64 buffers of this test's making"""
    from epgpy_amd import _lib
    dbuf, dptr, dstride = padded(ctx, m32.fl32(D), dpad, lead)
    sbuf, sptr, sstride = padded(ctx, m32.fl32(S), spad, lead)
    norms = _lib.signal_norms(ctx, dptr, dstride, D.shape[0], D.shape[1], c64=True)
    try:
        return _lib.signal_match(ctx, dptr, dstride, norms.ptr.value, D.shape[1], sptr, sstride, D.shape[0], S.shape[1], nsplit=nsplit,
                                 c64=True)
    finally:
        for b in (dbuf, sbuf, norms):
            b.free()


def same_bits(got, want):
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes()


def triple(res):
    return res.index, res.scale, res.score


@pytest.mark.parametrize("name", sorted(CASES))
def test_case_against_yardstick(name):
    """every shape, the record counts around the LDS chunk, the correlated dictionaries, the 1000-record case, ties and invalid
    atoms through match.match(match.Dictionary(D, dtype=complex64), S) on host arrays"""
    from epgpy_amd import match
    D, S = CASES[name]
    dic = match.Dictionary(D[:, :, None], dtype=C64)    # (a grid with a trailing axis of one: the flat index is unchanged)
    assert dic.dtype == C64 and dic.grid == (D.shape[1], 1)
    res = match.match(dic, S)
    assert res.index.shape == res.scale.shape == res.score.shape == (S.shape[1],)
    worst = yard(name).check(res.index, res.scale, res.score, what=name)
    print(name, "largest share of the bounds used:", worst)


def test_close_dictionary_within_the_slack():
    """decay_257_67_37: neighbouring atoms are closer than the float32 bound, so NO voxel of this case is decisive; asserted is
    only that the returned atom's q lies within the slack of the best"""
    from epgpy_amd import match
    D, S = m32.close_case()
    y = m32.Yardstick32(D, S)
    assert not y.decisive.any()
    res = match.match(match.Dictionary(D, dtype=C64), S)
    print("decay_257_67_37 largest share of the slack used:", y.check_slack(res.index, what="decay_257_67_37"))


@pytest.mark.parametrize("name", ["gauss_257_67_5", "gauss_33_67_37", "gauss_17_17_5", "tie", "gauss_33_17_1000", "gauss_33_17_129"])
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


def test_a_voxel_does_not_depend_on_strides_voxels_or_other_atoms(ctx):
    name = "gauss_33_67_37"
    D, S = CASES[name]
    dense = raw_match(ctx, D, S)
    yard(name).check(*dense, what=name)
    # rows padded with NaN columns and a NaN lead, both operands
    same_bits(raw_match(ctx, D, S, dpad=3, spad=5, lead=7), dense)
    same_bits(raw_match(ctx, D, S, dpad=1, spad=0, lead=1), dense)
    # the first 1, 16, 17 voxels of the 67 give the bits of the full call
    for name in ("gauss_33_67_37", "gauss_257_67_5", "decay_65_67_37"):
        D, S = CASES[name]
        full = raw_match(ctx, D, S)
        for k in (1, 16, 17):
            same_bits(raw_match(ctx, D, np.ascontiguousarray(S[:, :k])), [x[:k] for x in full])
        part = raw_match(ctx, D, np.ascontiguousarray(S[:, 40:41]))
        same_bits(part, [x[40:41] for x in full])
        # one atom tile less: the voxels whose best atom is elsewhere keep their bits
        keep = D.shape[1] - 16
        less = raw_match(ctx, np.ascontiguousarray(D[:, :keep]), S)
        stay = full[0] < keep
        assert stay.any() and not stay.all()
        same_bits([x[stay] for x in less], [x[stay] for x in full])


@pytest.mark.parametrize("shape", [(1, 1), (3, 65), (5, 257)])
def test_narrow_is_astype(ctx, shape):
    """epgx_signal_narrow on padded rows of both sides equals astype(np.complex64) bit for bit: +-0, float32 subnormals, halfway
    cases, values just above FLT_MAX (-> Inf), Inf; for NaN only that it stays one.  The padding of the output stays untouched"""
    from epgpy_amd import _lib
    vals = m32.narrow_values(shape)
    with np.errstate(over="ignore", invalid="ignore"):
        want = vals.astype(C64)
    nrow, ncol = shape
    sbuf, sptr, sstride = padded(ctx, vals, 3, lead=2)
    fill = np.full(5 + nrow * (ncol + 5), 7.0 - 3.0j, dtype=C64)
    obuf = _lib.DeviceBuffer(ctx, max(fill.nbytes, 16))
    obuf.upload(fill)
    _lib.signal_narrow_into(ctx, sptr, sstride, obuf.ptr.value + 8 * 5, ncol + 5, nrow, ncol)
    got_all = obuf.download(C64, fill.shape)
    src_after = sbuf.download(np.complex128, (2 + nrow * (ncol + 3),))
    got = got_all[5:].reshape(nrow, ncol + 5)
    assert (got_all[:5] == fill[:5]).all() and (got[:, ncol:] == 7.0 - 3.0j).all()
    g, w = np.ascontiguousarray(got[:, :ncol]).view(np.float32), want.view(np.float32)
    nan = np.isnan(w)
    assert (np.isnan(g) == nan).all()
    assert g[~nan].tobytes() == w[~nan].tobytes()
    assert np.ascontiguousarray(src_after[2:].reshape(nrow, ncol + 3)[:, :ncol]).view(np.float64)[~np.isnan(vals.view(np.float64))].tobytes() \
        == vals.view(np.float64)[~np.isnan(vals.view(np.float64))].tobytes()
    dense = _lib.signal_narrow(ctx, sptr, sstride, nrow, ncol)
    d = dense.download(C64, shape).view(np.float32)
    assert (np.isnan(d) == nan).all() and d[~nan].tobytes() == w[~nan].tobytes()
    for b in (sbuf, obuf, dense):
        b.free()


def test_norms_and_an_atom_that_overflows(ctx):
    from epgpy_amd import match
    D, _ = CASES["gauss_257_67_5"]
    dic = match.Dictionary(D, dtype=C64)
    assert dic.grid == (257,) and dic.natoms == 257 and dic.nrec == 5 and dic.dtype == C64
    got = dic.norms
    assert got.shape == (257,) and got.dtype == np.float64
    print("norms: largest share of the float64 bound used:", yard("gauss_257_67_5").check_norms(got))
    D, _ = CASES["gauss_33_17_1000"]
    print("norms, 1000 records:", yard("gauss_33_17_1000").check_norms(match.Dictionary(D, dtype=C64).norms))

    D, S, _ = mc.invalid_case()
    D = D.copy()
    D[0, 5] = 3.5e38                       # finite in complex128, Inf once rounded: the atom is invalid
    y = m32.Yardstick32(D, S)
    assert list(np.flatnonzero(~y.valid)) == [3, 5, 8, 16]
    dic = match.Dictionary(D, dtype=C64)
    y.check_norms(dic.norms)
    assert np.isinf(dic.norms[5]) and dic.norms[3] == 0 and np.isnan(dic.norms[16])
    for nsplit in (0, 1, 3, 17):
        res = match.match(dic, S, nsplit=nsplit)
        assert not np.isin(res.index, [3, 5, 8, 16]).any() and (res.index >= 0).all()
        assert res.score[4] == 0.0 and res.scale[4] == 0.0 and np.isfinite(res.score).all() and np.isfinite(res.scale).all()
        y.check(*triple(res))


def test_host_route_equals_device_route(ctx):
    """Dictionary(array, dtype=complex64) (astype on the host, uploaded at 8 bytes) and a DeviceSignal over a complex128 buffer
    narrowed on the device -- by Dictionary(handle, dtype=complex64) and by .astype -- hold the same bits, give the same norms
    and the same matches; the complex128 buffer is not modified.  Signals on the device are narrowed there to the same bits"""
    from epgpy_amd import match, functions, _lib
    name = "gauss_33_67_37"
    D, S = CASES[name]
    nrec = D.shape[0]
    host = match.Dictionary(D.reshape(nrec, 3, 11), dtype=C64)
    dbuf = _lib.DeviceBuffer(ctx, D.nbytes)
    dbuf.upload(D)
    dsig = functions.DeviceSignal(dbuf, nrec, (3, 11), 0, 1)
    wide = match.Dictionary(dsig)
    assert wide.dtype == np.complex128 and wide.astype(np.complex128) is wide and wide.astype(None) is wide
    routes = [match.Dictionary(dsig, dtype=C64), wide.astype(C64), wide.astype("complex64")]
    want = host.download()
    assert want.dtype == C64 and want.shape == (nrec, 3, 11) and want.tobytes() == m32.fl32(D).tobytes()
    ref = match.match(host, S)
    yard(name).check(*triple(ref), what=name)
    sbuf = _lib.DeviceBuffer(ctx, S.nbytes)
    sbuf.upload(S)
    ssig = functions.DeviceSignal(sbuf, nrec, (67,), 0, 1)
    for dev in routes:
        assert dev.dtype == C64 and dev.grid == (3, 11) and dev is not wide
        assert dev.download().tobytes() == want.tobytes()
        assert dev.norms.tobytes() == host.norms.tobytes()
        same_bits(triple(match.match(dev, S)), triple(ref))
        same_bits(triple(match.match(dev, ssig)), triple(ref))
        with pytest.raises(NotImplementedError, match="download"):
            dev.records
        with pytest.raises(NotImplementedError):
            dev.astype(np.complex128)
    assert dbuf.download(np.complex128, D.shape).tobytes() == D.tobytes()
    assert sbuf.download(np.complex128, S.shape).tobytes() == S.tobytes()
    assert np.asarray(wide.records).tobytes() == D.tobytes() and wide.download().tobytes() == D.tobytes()
    same_bits(triple(match.match(wide, S)), triple(match.match(D, S)))            # the complex128 path is the one it was
    # special values go the same way on both routes
    vals = m32.narrow_values((5, 257))
    vbuf = _lib.DeviceBuffer(ctx, vals.nbytes)
    vbuf.upload(vals)
    a = match.Dictionary(vals, dtype=C64)
    b = match.Dictionary(functions.DeviceSignal(vbuf, 5, (257,), 0, 1), dtype=C64)
    ga, gb = a.download().view(np.float32), b.download().view(np.float32)
    nan = np.isnan(ga)
    assert (np.isnan(gb) == nan).all() and ga[~nan].tobytes() == gb[~nan].tobytes()
    na, nb = a.norms, b.norms
    assert (np.isnan(na) == np.isnan(nb)).all() and na[~np.isnan(na)].tobytes() == nb[~np.isnan(nb)].tobytes()
    with pytest.raises(ValueError, match="device"):
        match.match(host, functions.DeviceSignal(_OtherBuf(), nrec, (67,), 0, 1))


class _OtherBuf:
    """a buffer of another context: the mismatch is refused before anything touches it"""
    class ctx:
        device = 0
    class ptr:
        value = 1 << 20


def test_compress_to_complex64(ctx):
    from epgpy_amd import match
    D, S, rank = cc.compressed_cases()["gauss_257_67_37"]
    wide = match.compress(D, rank=rank)
    basis = match.compress(D, rank=rank, dtype=C64)
    assert basis.U.tobytes() == wide.U.tobytes() and basis.s.tobytes() == wide.s.tobytes() and basis.energy == wide.energy
    cdic = basis.dictionary
    assert cdic.dtype == C64 and cdic.basis is basis and cdic.nrec == rank and cdic.grid == (257,)
    Dc = np.asarray(wide.dictionary.records)
    assert cdic.download().tobytes() == Dc.astype(C64).tobytes()
    again = wide.dictionary.astype(C64)
    assert again.basis is wide and again.download().tobytes() == cdic.download().tobytes()
    with pytest.raises(NotImplementedError, match="complex64"):
        match.compress(cdic, rank=2)
    # unprojected signals: projected in float64 on the device, then rounded; the yardstick on those rounded projected operands
    Sc = np.asarray(wide.project(S))
    y = m32.Yardstick32(Dc.reshape(rank, 257), Sc.reshape(rank, -1))
    res = match.match(cdic, S)
    print("compressed, rank", rank, "largest share of the bounds used:", y.check(*triple(res), what="compressed"))
    same_bits(triple(match.match(again, S)), triple(res))
    if rank != D.shape[0]:
        same_bits(triple(match.match(cdic, Sc)), triple(res))        # signals of `rank` records are taken as projected
    with pytest.raises(ValueError, match="records"):
        match.match(cdic, S[:5])


def test_end_to_end_from_the_simulator(ctx):
    """8 x 9 (T2, B1) multi-spin-echo dictionary of 12 echoes left on the device, narrowed there; signals are noisy scaled copies
    of chosen atoms: the true atoms come back and scale is the planted proton density up to the noise and the yardstick's bound"""
    from epgpy_amd import epg, match, functions
    T2 = np.geomspace(30.0, 200.0, 8)[:, None]
    B1 = np.linspace(0.7, 1.2, 9)[None, :]
    rlx = epg.E(5.0, 1000.0, T2)
    seq = [epg.T(90.0 * B1, 90)] + [epg.S(1), rlx, epg.T(150.0 * B1, 0), epg.S(1), rlx, epg.ADC] * 12
    handle = epg.simulate(seq, out="device")
    if isinstance(handle, (tuple, list)):
        handle = handle[0]
    assert isinstance(handle, functions.DeviceSignal) and handle.shape == (12, 8, 9)
    D = np.asarray(handle).reshape(12, 72)
    dic = match.Dictionary(handle, dtype=C64)
    assert dic.dtype == C64 and dic.grid == (8, 9) and dic.download().tobytes() == m32.fl32(D).reshape(12, 8, 9).tobytes()
    assert np.asarray(handle).tobytes() == D.tobytes()

    rng = np.random.default_rng(23)
    # atom = 9 i(T2) + i(B1), i(B1) <= 6: at B1 = 1.2 the refocusing angle is 180 degrees, where the signal does not change with
    # B1 to first order and neighbouring atoms are closer than the float32 bound
    atoms = np.array([0, 4, 9, 15, 20, 24, 31, 33, 40, 51, 58, 63, 69])
    pd = (0.5 + rng.random(len(atoms))) * np.exp(2j * np.pi * rng.random(len(atoms)))
    noise = 1e-3 * np.sqrt(np.mean(np.abs(D) ** 2))
    S = pd[None, :] * D[:, atoms] + noise * (rng.standard_normal((12, len(atoms))) + 1j * rng.standard_normal((12, len(atoms))))
    res = match.match(dic, S)
    y = m32.Yardstick32(D, S)
    assert y.decisive.all() and (y.amax == atoms).all()
    print("mse, complex64: largest share of the bounds used:", y.check(*triple(res), what="mse"))
    assert (res.index == atoms).all()
    i1, i2 = res.unravel()
    w1, w2 = np.unravel_index(atoms, (8, 9))
    assert (i1 == w1).all() and (i2 == w2).all()
    m = np.arange(len(atoms))
    ref = y.c[atoms, m] / y.n[atoms]                                   # what an exact evaluation on the rounded operands gives
    off = np.abs(ref - pd)                                             # the noise and the rounding of the operands: not the device's
    assert float(off.max()) < 5e-3
    tol = (y.bc[atoms, m] + y.g * y.absc[atoms, m]) / y.n[atoms]
    assert np.all(np.abs(res.scale.astype(np.clongdouble) - pd) <= tol + off)
    same_bits(triple(match.match(match.Dictionary(D.reshape(12, 8, 9), dtype=C64), S)), triple(res))


def test_result_types_zero_signals_and_invalid_only_dictionaries(ctx):
    from epgpy_amd import match
    D, S = CASES["gauss_17_17_5"]
    dic = match.Dictionary(D, dtype=C64)
    wide = match.match(D, S)
    res = match.match(dic, S)
    for a, b in zip(triple(res), triple(wide)):
        assert a.dtype == b.dtype and a.shape == b.shape
    assert res.index.dtype == np.int64 and res.scale.dtype == np.complex128 and res.score.dtype == np.float64 and res.grid == (17,)
    real = np.ascontiguousarray(S.real[:, :12]).reshape(5, 3, 4)
    shaped = match.match(dic, real)
    assert shaped.index.shape == (3, 4) and shaped.scale.dtype == np.complex128
    m32.Yardstick32(D, real.reshape(5, 12).astype(np.complex128)).check(*triple(shaped))
    one = match.match(dic, S[:, 3])
    assert one.index.shape == () and one.index == res.index[3] and one.scale == res.scale[3] and one.score == res.score[3]
    empty = match.match(dic, np.zeros((5, 0)))
    assert empty.index.shape == (0,) and empty.score.shape == (0,)
    zero = match.match(dic, np.zeros((5, 3)))
    assert (zero.score == 0).all() and (zero.scale == 0).all() and (zero.index >= 0).all()
    tiny = match.match(dic, np.full((5, 2), 1e-60))                  # rounds to an all-zero complex64 signal
    assert (tiny.score == 0).all() and (tiny.scale == 0).all()
    none = np.zeros((5, 17), dtype=np.complex128)
    none[1, ::2] = np.nan
    none[2, 1] = 1e39                                                 # Inf once rounded
    res = match.match(match.Dictionary(none, dtype=C64), S)
    assert (res.index == -1).all() and (res.scale == 0).all() and (res.score == 0).all()
    assert all((ax == -1).all() for ax in res.unravel())


def test_freed_buffer_gives_the_library_error(ctx):
    from epgpy_amd import match, functions, _lib
    D, S = CASES["gauss_17_17_5"]
    buf = _lib.DeviceBuffer(ctx, D.nbytes)
    buf.upload(D)
    sig = functions.DeviceSignal(buf, 5, (17,), 0, 1)
    dic = match.Dictionary(sig, dtype=C64)
    buf.free()
    res = match.match(dic, S)                    # the complex64 dictionary owns its records: the source is not kept alive
    m32.Yardstick32(D, S).check(*triple(res))
    with pytest.raises(_lib.EpgxError):
        match.Dictionary(sig, dtype=C64)


def test_entry_point_errors(ctx):
    """every EPGX_ERR_INVALID condition of include/epgx.h through raw calls: -1, a message, nothing launched"""
    import ctypes
    from epgpy_amd import _lib
    lib = ctx.lib
    natoms, nmeas, nrec = 17, 15, 5
    D, S = CASES["gauss_17_17_5"]
    D, S = m32.fl32(D), np.ascontiguousarray(m32.fl32(S)[:, :nmeas])
    dbuf, sbuf = _lib.DeviceBuffer(ctx, D.nbytes), _lib.DeviceBuffer(ctx, S.nbytes)
    dbuf.upload(D)
    sbuf.upload(S)
    nbuf = _lib.DeviceBuffer(ctx, 8 * natoms, itemsize=8)
    out = _lib.DeviceBuffer(ctx, 32 * nmeas, itemsize=8)
    d, s, n, o = dbuf.ptr.value, sbuf.ptr.value, nbuf.ptr.value, out.ptr.value
    P = ctypes.c_void_p

    def norms(dict_=d, stride=natoms, nrec_=nrec, natoms_=natoms, out_=n):
        return lib.epgx_signal_norms_c64(ctx.handle, P(dict_) if dict_ else None, stride, nrec_, natoms_, P(out_) if out_ else None)

    def run(dict_=d, dstride=natoms, norms_=n, natoms_=natoms, sig=s, sstride=nmeas, nrec_=nrec, nmeas_=nmeas, nsplit=0,
            index=o + 16 * nmeas, scale=o, score=o + 24 * nmeas):
        p = lambda v: P(v) if v else None      # noqa: E731
        return lib.epgx_signal_match_c64(ctx.handle, p(dict_), dstride, p(norms_), natoms_, p(sig), sstride, nrec_, nmeas_, nsplit,
                                         p(index), p(scale), p(score))

    assert norms() == 0 and run() == 0
    ctx.synchronize()
    good = out.download(np.float64, (4 * nmeas,)).copy()
    m32.Yardstick32(D, S).check(good[2 * nmeas:3 * nmeas].view(np.int64), good[:2 * nmeas].view(np.complex128), good[3 * nmeas:])
    assert norms(dict_=d + 8, stride=natoms, natoms_=natoms - 1) == 0            # complex64 pointers are aligned to 8 bytes
    assert norms() == 0
    big = 1 << 62
    bad_norms = [dict(dict_=0), dict(out_=0), dict(dict_=d + 4), dict(out_=n + 4), dict(nrec_=0), dict(natoms_=0), dict(natoms_=-1),
                 dict(stride=natoms - 1), dict(stride=big, nrec_=2 ** 31 - 1)]
    for kw in bad_norms:
        assert norms(**kw) == -1, kw
        assert b"epgx_signal_norms_c64" in lib.epgx_last_error()
    bad_match = [dict(dict_=0), dict(norms_=0), dict(sig=0), dict(index=0), dict(scale=0), dict(score=0),
                 dict(dict_=d + 4), dict(sig=s + 4), dict(scale=o + 8), dict(norms_=n + 4), dict(index=o + 16 * nmeas + 4),
                 dict(score=o + 24 * nmeas + 4), dict(nrec_=0), dict(nrec_=-3), dict(natoms_=0), dict(nmeas_=-1), dict(nsplit=-1),
                 dict(nsplit=natoms + 1), dict(dstride=natoms - 1), dict(sstride=nmeas - 1), dict(dstride=big, nrec_=2 ** 31 - 1),
                 dict(sstride=big, nrec_=2 ** 31 - 1)]
    for kw in bad_match:
        assert run(**kw) == -1, kw
        assert b"epgx_signal_match_c64" in lib.epgx_last_error()
    assert run(nmeas_=0) == 0 and run(nmeas_=0, sstride=0) == 0          # nothing to do
    assert run(nsplit=natoms) == 0
    ctx.synchronize()
    assert out.download(np.float64, (4 * nmeas,)).tobytes() == good.tobytes()      # the refused calls wrote nothing
    for b in (dbuf, sbuf, nbuf, out):
        b.free()

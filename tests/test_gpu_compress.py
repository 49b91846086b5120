"""GPU: match.compress (gram_kernel, gram_reduce_kernel, project_kernel of csrc/epgx_compress.hip) against the extended-precision
yardstick of tests/compress_cases.py, whose bounds are derived there and not measured.  Shapes sit around the 16 x 16 x 4 MFMA
tile, the 64-record block and 16-atom LDS chunk of gram_kernel, the 16-record group and the column blocks of project_kernel and
the 1024 atoms at which the library's own nsplit changes; tests/test_compress_host.py checks the host half on the CPU."""
import ctypes

import numpy as np
import pytest

from tests import match_cases as mc
from tests import compress_cases as cc

pytestmark = pytest.mark.gpu

CASES = cc.cases()
_BASIS = {}


def host_basis(name):
    if name not in _BASIS:
        _BASIS[name] = cc.host_basis(CASES[name][0])
    return _BASIS[name]


@pytest.fixture(scope="module")
def ctx():
    from epgpy_amd import _lib
    return _lib.get_context()


def padded(ctx, A, pad, lead=0):
    """A [nrec, ncol] in a device buffer with rows of ncol + pad elements, `lead` elements in; padding and lead hold NaN"""
    from epgpy_amd import _lib
    nrec, ncol = A.shape
    host = np.full(lead + nrec * (ncol + pad), np.nan + 1j * np.nan, dtype=np.complex128)
    host[lead:].reshape(nrec, ncol + pad)[:, :ncol] = A
    buf = _lib.DeviceBuffer(ctx, host.nbytes)
    buf.upload(host)
    return buf, buf.ptr.value + 16 * lead, ncol + pad


def raw_gram(ctx, D, nsplit=0, pad=0, lead=0):
    from epgpy_amd import _lib
    dbuf, dptr, dstride = padded(ctx, D, pad, lead)
    norms = _lib.signal_norms(ctx, dptr, dstride, D.shape[0], D.shape[1])
    out = _lib.signal_gram(ctx, dptr, dstride, norms.ptr.value, D.shape[0], D.shape[1], nsplit=nsplit)
    try:
        return out.download(np.complex128, (D.shape[0], D.shape[0]))
    finally:
        for b in (dbuf, norms, out):
            b.free()


def raw_project(ctx, B, X, pad=0, lead=0):
    from epgpy_amd import _lib
    B = np.ascontiguousarray(B)
    bbuf = _lib.DeviceBuffer(ctx, B.nbytes)
    bbuf.upload(B)
    xbuf, xptr, xstride = padded(ctx, X, pad, lead)
    out = _lib.signal_project(ctx, bbuf.ptr.value, B.shape[1], xptr, xstride, X.shape[0], X.shape[1])
    try:
        return out.download(np.complex128, (B.shape[1], X.shape[1]))
    finally:
        for b in (bbuf, xbuf, out):
            b.free()


@pytest.mark.parametrize("name", sorted(CASES))
def test_gram_against_yardstick(ctx, name):
    """every case within the bound; G bitwise Hermitian with a zero imaginary diagonal; the same bits in a second call; the
    library's nsplit = 0 is the documented rule; padded strides and a lead offset change no bit"""
    from epgpy_amd import _lib
    D, _ = CASES[name]
    G = raw_gram(ctx, D)
    print(name, "largest share of the Gram bound used:", cc.check_gram(G, D, name))
    assert (G.imag.diagonal() == 0).all() and not np.signbit(G.imag.diagonal()).any()
    upper, lower = G[np.triu_indices(len(G), 1)], G.T[np.triu_indices(len(G), 1)]
    assert upper.real.tobytes() == lower.real.tobytes() and upper.imag.tobytes() == (-lower.imag).tobytes()
    assert raw_gram(ctx, D).tobytes() == G.tobytes()
    assert raw_gram(ctx, D, nsplit=_lib.gram_nsplit(*D.shape)).tobytes() == G.tobytes()
    assert raw_gram(ctx, D, pad=3, lead=7).tobytes() == G.tobytes()


@pytest.mark.parametrize("name", ["gauss_257_5", "gauss_33_37", "gauss_17_5", "gauss_257_65", "gauss_2048_5", "gauss_33_1000", "invalid"])
def test_gram_forced_splits(ctx, name):
    D, _ = CASES[name]
    for nsplit in (1, 2, 3, D.shape[1]):
        G = raw_gram(ctx, D, nsplit=nsplit)
        cc.check_gram(G, D, f"{name} nsplit={nsplit}")
        assert (G.imag.diagonal() == 0).all() and (G == G.conj().T).all()


def test_gram_ignores_what_invalid_atoms_hold(ctx):
    """atom 3 all zero, atom 16 a NaN, atom 8 an Inf: G is finite and is the Gram matrix of the other columns, bit for bit
    whatever the invalid columns hold"""
    D, _ = cc.invalid_case()
    G = raw_gram(ctx, D)
    assert np.isfinite(G).all()
    cc.check_gram(G, D, "invalid")
    other = D.copy()
    other[:, 16] = np.inf
    other[:, 8] = -np.nan
    other[4, 3] = np.nan
    assert raw_gram(ctx, other).tobytes() == G.tobytes()


@pytest.mark.parametrize("name", sorted(n for n in CASES if n != "invalid"))
def test_project_against_yardstick(ctx, name):
    """every (case, rank) with a U from the host half: the dictionary's columns and the measured signals"""
    D, S = CASES[name]
    U = host_basis(name)
    for rank in cc.ranks_for(D.shape[0]):
        B = np.ascontiguousarray(U[:, :rank])
        for X, what in ((D, "dictionary"), (S, "signals")):
            worst = cc.check_project(raw_project(ctx, B, X), B, X, f"{name} rank {rank} {what}")
        print(name, "rank", rank, "largest share of the project bound used:", worst)


def test_project_bits_do_not_depend_on_the_call(ctx):
    """columns [5:22] alone and one column alone give the bits they have inside the full call; rank 4 is the first 4 rows of
    rank 17; padded row strides and a lead offset (NaN in the padding) change nothing"""
    for name in ("gauss_257_65", "gauss_33_37", "gauss_1025_17"):
        D, _ = CASES[name]
        U = host_basis(name)
        B17, B4 = np.ascontiguousarray(U[:, :17]), np.ascontiguousarray(U[:, :4])
        full = raw_project(ctx, B17, D)
        assert raw_project(ctx, B17, D[:, 5:22]).tobytes() == np.ascontiguousarray(full[:, 5:22]).tobytes()
        assert raw_project(ctx, B17, D[:, 20:21]).tobytes() == np.ascontiguousarray(full[:, 20:21]).tobytes()
        assert raw_project(ctx, B4, D).tobytes() == np.ascontiguousarray(full[:4]).tobytes()
        assert raw_project(ctx, B17, D, pad=3, lead=7).tobytes() == full.tobytes()
        if D.shape[0] >= 64:
            full64 = raw_project(ctx, np.ascontiguousarray(U[:, :64]), D)
            assert np.ascontiguousarray(full64[:17]).tobytes() == full.tobytes()
            full33 = raw_project(ctx, np.ascontiguousarray(U[:, :33]), D)
            assert np.ascontiguousarray(full64[:33]).tobytes() == full33.tobytes()


def test_host_half_and_device(ctx):
    """match.compress returns exactly the U the host half gives on the downloaded device Gram; the compressed records meet the
    project bound; the attributes"""
    from epgpy_amd import match
    for name, rank in (("decay_257_37", 6), ("gauss_257_65", 17), ("gauss_33_1000", 16)):
        D, S = CASES[name]
        G = raw_gram(ctx, D)
        U, lam = match.gram_basis(G)
        basis = match.compress(D[:, :, None], rank=rank)
        assert basis.U.tobytes() == np.ascontiguousarray(U[:, :rank]).tobytes()
        assert basis.rank == rank and basis.nrec == D.shape[0] and basis.s.shape == (D.shape[0],)
        assert basis.s.tobytes() == np.sqrt(np.clip(lam, 0, None)).tobytes() and 0 < basis.energy <= 1
        cdic = basis.dictionary
        assert cdic.basis is basis and cdic.nrec == rank and cdic.grid == (D.shape[1], 1) and cdic.natoms == D.shape[1]
        Dc = np.asarray(cdic.records)
        assert Dc.shape == (rank, D.shape[1], 1)
        cc.check_project(Dc.reshape(rank, -1), basis.U, D, name)
        Sc = basis.project(S)
        assert Sc.shape == (rank, S.shape[1])
        cc.check_project(np.asarray(Sc), basis.U, S, name)
        by_energy = match.compress(match.Dictionary(D), energy=basis.energy * (1 - 1e-12))
        assert by_energy.rank <= rank and by_energy.U.tobytes() == np.ascontiguousarray(U[:, :by_energy.rank]).tobytes()


def test_invalid_atoms_stay_invalid(ctx):
    from epgpy_amd import match
    D, S = cc.invalid_case()
    basis = match.compress(D, rank=3)
    Dc = np.asarray(basis.dictionary.records)
    assert not np.isfinite(Dc[:, 16]).any() and not np.isfinite(Dc[:, 8]).any() and (Dc[:, 3] == 0).all()
    ok = cc.valid_atoms(D)
    assert np.isfinite(Dc[:, ok]).all()
    cc.check_project(np.ascontiguousarray(Dc[:, ok]), basis.U, D[:, ok], "invalid")
    norms = basis.dictionary.norms
    assert not np.isfinite(norms[[8, 16]]).any() and norms[3] == 0
    for nsplit in (0, 1, 3, 17):
        res = match.match(basis.dictionary, S, nsplit=nsplit)
        assert not np.isin(res.index, [3, 8, 16]).any()
    with pytest.raises(ValueError, match="no valid atom"):
        none = np.zeros((5, 17), dtype=np.complex128)
        none[1, ::2] = np.nan
        match.compress(none, rank=1)
    with pytest.raises(ValueError, match="largest resolvable rank is 3"):
        match.compress(cc.rank3_dictionary(), rank=5)


@pytest.mark.parametrize("name", sorted(cc.compressed_cases()))
def test_matching_in_the_compressed_space(ctx, name):
    """match.match(cdic, S) passes the yardstick of match_cases on (U^H D, U^H S) built on the host from the returned U and the
    downloaded Dc, and is bit-identical to matching the projected signals, on the device and from the host"""
    from epgpy_amd import match
    D, S, rank = cc.compressed_cases()[name]
    basis = match.compress(D, rank=rank)
    cdic = basis.dictionary
    res = match.match(cdic, S)
    Dc = np.asarray(cdic.records)
    Sc = np.asarray(basis.project(S))
    cc.check_project(Dc, basis.U, D, name)
    cc.check_project(Sc, basis.U, S, name)
    y = mc.Yardstick(Dc, Sc)
    assert y.decisive.mean() >= 0.9
    print(name, "largest share of the bounds used:", y.check(res.index, res.scale, res.score, what=name))
    for other in (match.match(cdic, basis.project(S)), match.match(Dc, Sc)):
        for g, w in ((other.index, res.index), (other.scale, res.scale), (other.score, res.score)):
            assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes()
    assert res.grid == (D.shape[1],)


def test_end_to_end_from_the_simulator(ctx):
    """8 x 9 (T1, T2) multi-spin-echo dictionary of 24 echoes left on the device, compressed with energy=0.9999 as a DeviceSignal
    and as a DeviceJacobian; signals simulated at 11 off-grid parameter pairs"""
    from epgpy_amd import epg, match, functions
    T1 = np.geomspace(400.0, 2000.0, 8)[:, None]
    T2 = np.geomspace(30.0, 200.0, 9)[None, :]

    def train(t1, t2, **kw):
        rlx = epg.E(5.0, t1, t2, **kw)
        return [epg.T(90, 90)] + [epg.S(1), rlx, epg.T(150, 0), epg.S(1), rlx, epg.ADC] * 24

    rng = np.random.default_rng(21)
    t1 = rng.uniform(450.0, 1900.0, 11)
    t2 = rng.uniform(35.0, 190.0, 11)
    pd = (0.5 + rng.random(11)) * np.exp(2j * np.pi * rng.random(11))
    S = np.asarray(epg.simulate(train(t1, t2))).reshape(24, 11) * pd

    handle = epg.simulate(train(T1, T2), out="device")
    if isinstance(handle, (tuple, list)):
        handle = handle[0]
    assert isinstance(handle, functions.DeviceSignal) and handle.shape == (24, 8, 9)
    jac = epg.simulate(train(T1, T2, order1=["T2"]), probe=epg.Jacobian(["magnitude", "T2"]), out="device")
    if isinstance(jac, (tuple, list)):
        jac = jac[0]
    assert isinstance(jac, functions.DeviceJacobian)
    for dic, D in ((handle, np.asarray(handle)), (jac, np.asarray(match._signal_handle(jac, "dictionary")))):
        D = D.reshape(24, 72)
        basis = match.compress(dic, energy=0.9999)
        assert 1 <= basis.rank < 24 and basis.energy >= 0.9999 and basis.nrec == 24
        lam = basis.s ** 2
        assert basis.rank == 1 or lam[:basis.rank - 1].sum() / lam.sum() < 0.9999
        cdic = basis.dictionary
        assert cdic.grid == (8, 9) and cdic.records.shape == (basis.rank, 8, 9)
        Dc = np.asarray(cdic.records).reshape(basis.rank, 72)
        cc.check_project(Dc, basis.U, D, "mse")
        res = match.match(cdic, S)
        Sc = np.asarray(basis.project(S))
        cc.check_project(Sc, basis.U, S, "mse signals")
        mc.Yardstick(Dc, Sc).check(res.index, res.scale, res.score, what="mse")
        i1, i2 = res.unravel()
        w1, w2 = np.unravel_index(res.index, (8, 9))
        assert (i1 == w1).all() and (i2 == w2).all() and res.grid == (8, 9)


def test_freed_buffer_gives_the_library_error(ctx):
    from epgpy_amd import match, functions, _lib
    D, _ = CASES["gauss_17_5"]
    buf = _lib.DeviceBuffer(ctx, D.nbytes)
    buf.upload(D)
    sig = functions.DeviceSignal(buf, 5, (17,), 0, 1)
    dic = match.Dictionary(sig)
    buf.free()
    with pytest.raises(_lib.EpgxError):
        match.compress(dic, rank=2)
    with pytest.raises(_lib.EpgxError):
        match.compress(sig, rank=2)


def test_entry_point_errors(ctx):
    """every EPGX_ERR_INVALID condition of both entries through raw calls: -1, a message, nothing written"""
    from epgpy_amd import _lib
    lib = ctx.lib
    natoms, nrec, rank = 17, 5, 3
    D, _ = CASES["gauss_17_5"]
    B = np.ascontiguousarray(host_basis("gauss_17_5")[:, :rank])
    dbuf, bbuf = _lib.DeviceBuffer(ctx, D.nbytes), _lib.DeviceBuffer(ctx, B.nbytes)
    dbuf.upload(D)
    bbuf.upload(B)
    nbuf = _lib.signal_norms(ctx, dbuf.ptr.value, natoms, nrec, natoms)
    gout = _lib.DeviceBuffer(ctx, 16 * nrec * nrec)
    pout = _lib.DeviceBuffer(ctx, 16 * rank * natoms)
    d, b, n, g, o = dbuf.ptr.value, bbuf.ptr.value, nbuf.ptr.value, gout.ptr.value, pout.ptr.value
    P = ctypes.c_void_p
    p = lambda v: P(v) if v else None      # noqa: E731

    def gram(dict_=d, stride=natoms, norms_=n, nrec_=nrec, natoms_=natoms, nsplit=0, out=g):
        return lib.epgx_signal_gram(ctx.handle, p(dict_), stride, p(norms_), nrec_, natoms_, nsplit, p(out))

    def project(basis=b, rank_=rank, src=d, sstride=natoms, nrec_=nrec, ncol=natoms, out=o, ostride=natoms):
        return lib.epgx_signal_project(ctx.handle, p(basis), rank_, p(src), sstride, nrec_, ncol, p(out), ostride)

    assert gram() == 0 and project() == 0
    ctx.synchronize()
    good_g = gout.download(np.complex128, (nrec, nrec)).copy()
    good_p = pout.download(np.complex128, (rank, natoms)).copy()
    cc.check_gram(good_g, D)
    cc.check_project(good_p, B, D)
    big = 1 << 62
    bad_gram = [dict(dict_=0), dict(norms_=0), dict(out=0), dict(dict_=d + 8), dict(out=g + 8), dict(norms_=n + 4), dict(nrec_=0),
                dict(nrec_=-2), dict(natoms_=0), dict(natoms_=-1), dict(nsplit=-1), dict(nsplit=natoms + 1), dict(stride=natoms - 1),
                dict(stride=big, nrec_=2 ** 31 - 1), dict(nrec_=2 ** 31 - 1, stride=natoms, nsplit=natoms)]
    for kw in bad_gram:
        assert gram(**kw) == -1, kw
        assert b"epgx_signal_gram" in lib.epgx_last_error()
    bad_project = [dict(basis=0), dict(src=0), dict(out=0), dict(basis=b + 8), dict(src=d + 8), dict(out=o + 8), dict(nrec_=0),
                   dict(nrec_=-1), dict(ncol=-1), dict(rank_=0), dict(rank_=-1), dict(rank_=65, nrec_=100), dict(rank_=nrec + 1),
                   dict(sstride=natoms - 1), dict(ostride=natoms - 1), dict(sstride=big, nrec_=2 ** 31 - 1), dict(ostride=big)]
    for kw in bad_project:
        assert project(**kw) == -1, kw
        assert b"epgx_signal_project" in lib.epgx_last_error()
    assert project(ncol=0) == 0 and project(ncol=0, sstride=0, ostride=0) == 0          # nothing to do
    ctx.synchronize()
    assert gout.download(np.complex128, (nrec, nrec)).tobytes() == good_g.tobytes()             # the refused calls wrote nothing
    assert pout.download(np.complex128, (rank, natoms)).tobytes() == good_p.tobytes()
    assert gram(nsplit=natoms) == 0
    ctx.synchronize()
    cc.check_gram(gout.download(np.complex128, (nrec, nrec)), D)
    for buf in (dbuf, bbuf, nbuf, gout, pout):
        buf.free()

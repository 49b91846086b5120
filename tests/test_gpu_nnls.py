"""GPU: epgpy_amd.match.Components / match.nnls (component_gram_kernel and nnls_kernel of csrc/epgx_nnls.hip through
epgx_signal_component_gram / epgx_signal_nnls) against the extended-precision yardstick of tests/nnls_cases.py, with
`scipy.optimize.nnls` and `match.nnls_host` as references and the MARGIN derived there.  tests/test_nnls_host.py shows on the CPU
that every regular case is solved (status 0) by the definition itself, that the passive set of two cases reaches all A atoms and
that atoms leave it in others.  The cap of 3 A solves (status 1) is held by the CPU test alone: no dictionary is known that
reaches it."""
import ctypes

import numpy as np
import pytest

from tests import nnls_cases as nc

pytestmark = pytest.mark.gpu

CASES = nc.cases()
_HOST, _DEV = {}, {}


@pytest.fixture(scope="module")
def ctx():
    from epgpy_amd import _lib
    return _lib.get_context()


def host(name):
    from epgpy_amd import match
    if name not in _HOST:
        c = CASES[name]
        _HOST[name] = match.nnls_host(c["D"], c["S"], c["axis"], reg=c["reg"])
    return _HOST[name]


def device(name):
    from epgpy_amd import match
    if name not in _DEV:
        c = CASES[name]
        comp = match.Components(c["D"], c["axis"])
        _DEV[name] = (comp, match.nnls(comp, c["S"], reg=c["reg"]))
    return _DEV[name]


def scipy_one(y, m, g, reg):
    """scipy's weights of voxel m in group g, on the stacked real system"""
    from scipy.optimize import nnls
    ok = y.valid[:, g]
    d = y.D[:, ok, g]
    mu = float(y.mu[g])
    M = np.concatenate([d.real, d.imag, np.sqrt(mu) * np.eye(int(ok.sum()))], axis=0)
    rhs = np.concatenate([y.S[:, m].real, y.S[:, m].imag, np.zeros(int(ok.sum()))])
    out = np.zeros(y.A)
    out[ok] = nnls(M, rhs, maxiter=30 * y.A)[0]
    return out


def same_bits(got, want):
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes()


def fields(res, cols=slice(None)):
    return (np.ascontiguousarray(res.weights.reshape(res.weights.shape[0], -1)[:, cols]), np.ascontiguousarray(res.group.reshape(-1)[cols]),
            np.ascontiguousarray(res.residual.reshape(-1)[cols]), np.ascontiguousarray(res.status.reshape(-1)[cols]))


@pytest.mark.parametrize("name", sorted(CASES))
def test_case_against_yardstick(name):
    """objective within MARGIN of scipy's and of nnls_host's, x >= 0 exactly, status 0 everywhere, the Gram matrices"""
    c = CASES[name]
    comp, res = device(name)
    ref = host(name)
    y = nc.Yardstick(c["D"], c["S"], c["axis"], c["reg"])
    A, nmeas = y.A, c["S"].shape[1]
    assert (comp.ncomp, comp.ngroups, comp.nrec, comp.axis) == (A, y.G, y.nrec, c["axis"])
    assert res.weights.shape == (A, nmeas) and res.group.shape == res.residual.shape == res.status.shape == (nmeas,)
    assert res.weights.dtype == np.float64 and res.group.dtype == np.int64 and res.status.dtype == np.int32
    assert (ref.status == 0).all() and (res.status == 0).all()
    assert (res.weights >= 0).all()
    H = comp.gram
    want = np.einsum("tag,tbg->gab", y.D.real, y.D.real) + np.einsum("tag,tbg->gab", y.D.imag, y.D.imag)
    assert H.tobytes() == np.swapaxes(H, 1, 2).tobytes(), "symmetric to the bit"
    scale = np.sqrt(np.einsum("gaa->ga", want))
    assert np.all(np.abs(H - want) <= 4 * y.nrec * 2.0 ** -53 * scale[:, :, None] * scale[:, None, :])
    assert comp.valid.all()
    cond = nc.cond_ridge(c["D"], c["axis"], c["reg"])
    worst = 0.0
    for m in range(nmeas):
        g = int(res.group[m])
        assert 0 <= g < y.G
        Jd = y.J(m, g, res.weights[:, m])
        Jh = y.J(m, int(ref.group[m]), ref.weights[:, m])
        sp = scipy_one(y, m, g, c["reg"])
        Js = y.J(m, g, sp)
        worst = max(worst, float(Jd / Js - 1), float(Jd / Jh - 1))
        assert Jd <= Js * (1 + nc.MARGIN), (name, m, float(Jd), float(Js))
        assert Jd <= Jh * (1 + nc.MARGIN), (name, m, float(Jd), float(Jh), "the best group")
        assert abs(res.residual[m] - float(y.residual(m, g, res.weights[:, m]))) <= nc.residual_tol(y.nrec, y.A, y.energy(m))
        if c["reg"] >= 1e-4:
            assert np.max(np.abs(res.weights[:, m] - sp)) <= nc.weight_tol(cond[g], sp), (name, m)
    print(name, "largest excess of J:", worst)
    if name.startswith("full"):
        assert ((res.weights > 0).sum(axis=0) == A).any(), "the passive set reaches all A atoms"


@pytest.mark.parametrize("name", ["a33_r33_g3_m130", "a64_r33_g3_m65", "axis_middle"])
def test_a_voxel_does_not_depend_on_the_others(name):
    """a voxel alone, in the permuted call and in the full call: the same bytes; so with its group fixed"""
    from epgpy_amd import match
    c = CASES[name]
    comp, full = device(name)
    nmeas = c["S"].shape[1]
    perm = np.random.default_rng(5).permutation(nmeas)
    mixed = match.nnls(comp, np.ascontiguousarray(c["S"][:, perm]), reg=c["reg"])
    same_bits(fields(mixed), fields(full, perm))
    for m in (0, nmeas // 2, nmeas - 1):
        one = match.nnls(comp, c["S"][:, m], reg=c["reg"])
        assert one.group.shape == () and one.weights.shape == (comp.ncomp,)
        same_bits(fields(one), fields(full, slice(m, m + 1)))
    fixed = match.nnls(comp, c["S"], reg=c["reg"], group=full.group)
    same_bits(fields(fixed), fields(full))
    other = (full.group + 1) % comp.ngroups
    moved = match.nnls(comp, c["S"], reg=c["reg"], group=other)
    assert (moved.group == other).all() and (moved.status == 0).all() and (moved.weights >= 0).all()


def test_degenerates_and_group_search():
    from epgpy_amd import match
    c = nc.special()
    D, S = c["D"], c["S"]
    comp = match.Components(D, 0)
    valid = comp.valid
    assert valid[0].all() and valid[3].all() and valid[1].tolist() == [True, True, False, True, False, True] and not valid[2].any()
    res = match.nnls(comp, S, reg=c["reg"])
    ref = match.nnls_host(D, S, 0, reg=c["reg"])
    y = nc.Yardstick(D, S, 0, c["reg"])
    assert (res.weights[:, 0] == 0).all() and res.status[0] == 0 and res.residual[0] == 0 and res.group[0] == 0      # all-zero signal
    assert res.group.tolist() == ref.group.tolist() == [0, 1, 1, 1, 0, 0, 0]         # groups 0 and 3 are equal: the lower index
    assert (res.status == 0).all() and np.isfinite(res.weights).all() and (res.weights >= 0).all()
    assert (res.weights[[2, 4], 1:4] == 0).all()                                     # the NaN atom and the all-zero atom
    for m in range(1, 7):
        g = int(res.group[m])
        assert y.J(m, g, res.weights[:, m]) <= y.J(m, g, ref.weights[:, m]) * (1 + nc.MARGIN)
    grp = np.array([3, 1, 1, 0, 3, 0, 2])
    fixed = match.nnls(comp, S, reg=c["reg"], group=grp)
    assert fixed.group.tolist() == grp.tolist() and (fixed.status == 0).all()
    same_bits(fields(fixed, [1, 2, 5]), fields(res, [1, 2, 5]))
    assert fixed.weights[:, 4].tobytes() == res.weights[:, 4].tobytes()              # group 3 holds the atoms of group 0
    assert (fixed.weights[:, 6] == 0).all()                                          # a group whose atoms are all invalid
    assert abs(fixed.residual[6] - np.linalg.norm(S[:, 6])) <= 1e-12 * np.linalg.norm(S[:, 6])
    out = match.nnls(comp, S, reg=c["reg"], group=np.array([-1, 4, 0, 0, 0, 0, 2 ** 40]))
    assert out.group[[0, 1, 6]].tolist() == [-1, -1, -1] and np.isnan(out.weights[:, [0, 1, 6]]).all()
    assert np.isnan(out.residual[[0, 1, 6]]).all() and (out.status[[0, 1, 6]] == 2).all()
    same_bits(fields(out, [4, 5]), fields(res, [4, 5]))
    bad = S.copy()
    bad[3, 2] = np.nan
    bad[0, 5] = np.inf
    out = match.nnls(comp, bad, reg=c["reg"])
    assert out.group[[2, 5]].tolist() == [-1, -1] and (out.status[[2, 5]] == 2).all() and np.isnan(out.weights[:, [2, 5]]).all()
    same_bits(fields(out, [1, 3, 4, 6]), fields(res, [1, 3, 4, 6]))


def test_shapes_real_signals_and_empty():
    from epgpy_amd import match
    c = CASES["axis_middle"]
    comp, flat = device("axis_middle")
    assert comp.grid == (3, 5, 2) and comp.groups == (3, 2)
    S = c["S"][:, :60]
    res = match.nnls(comp, S.reshape(8, 4, 15), reg=c["reg"])
    assert res.weights.shape == (5, 4, 15) and res.group.shape == (4, 15) and res.groups == (3, 2)
    same_bits(fields(res), fields(flat, slice(0, 60)))
    i, j = res.unravel()
    assert (i * 2 + j == res.group).all()
    t2 = np.geomspace(10.0, 100.0, 5)
    assert np.all((res.fraction(0.0, 30.0, t2) >= 0) & (res.fraction(0.0, 30.0, t2) <= 1)) and res.gmean(t2).shape == (4, 15)
    real = match.nnls(comp, np.ascontiguousarray(S.real), reg=c["reg"])
    wide = match.nnls(comp, S.real.astype(np.complex128), reg=c["reg"])
    same_bits(fields(real), fields(wide))
    empty = match.nnls(comp, np.zeros((8, 0)), reg=c["reg"])
    assert empty.weights.shape == (5, 0) and empty.group.shape == (0,)


def test_handles(ctx):
    """the dictionary as a DeviceSignal whose records lie three rows apart among NaN rows, as a DeviceJacobian, as a Dictionary;
    the signals as a DeviceSignal"""
    from epgpy_amd import match, functions, _lib
    c = CASES["axis_last"]
    D, S = c["D"], c["S"]
    comp, want = device("axis_last")
    nrec, grid, nvox = D.shape[0], D.shape[1:], int(np.prod(D.shape[1:]))
    hostbuf = np.full((nrec * 3, nvox), np.nan + 1j * np.nan, dtype=np.complex128)
    hostbuf[1::3] = D.reshape(nrec, nvox)
    buf = _lib.DeviceBuffer(ctx, hostbuf.nbytes)
    buf.upload(hostbuf)
    sig = functions.DeviceSignal(buf, nrec * 3, grid, 1, 3)
    assert sig.row_stride == 3 * nvox
    strided = match.Components(sig, 2)
    assert strided.gram.tobytes() == comp.gram.tobytes()
    same_bits(fields(match.nnls(strided, S, reg=c["reg"])), fields(want))

    jac = functions.DeviceJacobian(buf, nrec, grid, 1, 3, 0, [1, 2], ["x", "y"])       # row 0 of every record is NaN here ...
    hostbuf[0::3] = D.reshape(nrec, nvox)
    hostbuf[1::3] = np.nan
    buf.upload(hostbuf)                                                                  # ... and the dictionary now
    fromjac = match.Components(jac, -1)
    assert fromjac.axis == 2
    sbuf = _lib.DeviceBuffer(ctx, S.nbytes)
    sbuf.upload(S)
    dsig = functions.DeviceSignal(sbuf, nrec, (S.shape[1],), 0, 1)
    same_bits(fields(match.nnls(fromjac, dsig, reg=c["reg"])), fields(want))
    same_bits(fields(match.nnls(match.Components(match.Dictionary(D), 2), dsig, reg=c["reg"])), fields(want))

    with pytest.raises(NotImplementedError, match="complex64"):
        match.Components(match.Dictionary(D, dtype=np.complex64), 2)
    with pytest.raises(NotImplementedError, match="compressed"):
        match.Components(match.compress(match.Dictionary(D.reshape(nrec, nvox)), rank=2).dictionary, 0)
    with pytest.raises(NotImplementedError, match="slab"):
        match.Components(functions.DeviceSignal(buf, nrec * 3, grid, 1, 3, vox0=0, count=nvox - 1), 2)
    with pytest.raises(ValueError, match="records"):
        match.nnls(comp, S[:5])
    buf.free()
    with pytest.raises(_lib.EpgxError):
        match.Components(sig, 2)


def test_a_pivot_that_is_not_positive(ctx):
    """status 2 through the raw entry with a hand-made H: atom 0 enters, then atom 1 at the pivot 1 - 4"""
    from epgpy_amd import _lib
    D = np.array([[1.0, 0.5]], dtype=np.complex128)
    S = np.array([[1.0, 1.0]], dtype=np.complex128)
    H = np.array([[[1.0, -2.0], [-2.0, 1.0]], [[1.0, 0.0], [0.0, 0.25]]])
    dbuf, sbuf = _lib.DeviceBuffer(ctx, D.nbytes), _lib.DeviceBuffer(ctx, S.nbytes)
    hbuf, mbuf = _lib.DeviceBuffer(ctx, H.nbytes, itemsize=8), _lib.DeviceBuffer(ctx, 16, itemsize=8)
    dbuf.upload(D)
    sbuf.upload(S)
    hbuf.upload(H)
    mbuf.upload(np.array([3, 3], dtype=np.uint64))
    try:
        # one group of two atoms, two voxels: first with the indefinite H, then with the sound one that lies behind it
        w, g, r, st = _lib.signal_nnls(ctx, dbuf.ptr.value, 2, 1, 2, 1, 1, 1, hbuf.ptr.value, mbuf.ptr.value, sbuf.ptr.value, 2, 2, 0.0, 1e-10)
        assert g.tolist() == [-1, -1] and st.tolist() == [2, 2] and np.isnan(w).all() and np.isnan(r).all()
        w, g, r, st = _lib.signal_nnls(ctx, dbuf.ptr.value, 2, 1, 2, 1, 1, 1, hbuf.ptr.value + 32, mbuf.ptr.value + 8, sbuf.ptr.value, 2, 2,
                                       0.0, 1e-10)
        assert g.tolist() == [0, 0] and st.tolist() == [0, 0] and np.allclose(w, [[1.0, 1.0], [2.0, 2.0]], rtol=1e-15, atol=0)
    finally:
        for b in (dbuf, sbuf, hbuf, mbuf):
            b.free()


def test_entry_point_errors(ctx):
    """every EPGX_ERR_INVALID condition of include/epgx.h through raw calls: -1, a message that names the entry, nothing launched"""
    from epgpy_amd import _lib
    lib = ctx.lib
    c = CASES["a3_r8_g3_m65"]
    D, S = c["D"].reshape(8, 9), c["S"]
    nrec, A, G, nmeas = 8, 3, 3, 65
    dbuf, sbuf = _lib.DeviceBuffer(ctx, D.nbytes), _lib.DeviceBuffer(ctx, S.nbytes)
    dbuf.upload(D)
    sbuf.upload(S)
    hbuf, mbuf = _lib.DeviceBuffer(ctx, 8 * G * A * A, itemsize=8), _lib.DeviceBuffer(ctx, 8 * G, itemsize=8)
    gbuf = _lib.DeviceBuffer(ctx, 8 * nmeas, itemsize=8)
    gbuf.upload(np.zeros(nmeas, dtype=np.int64))
    out = _lib.DeviceBuffer(ctx, 8 * (A + 3) * nmeas, itemsize=8)
    d, s, h, k, gr, o = (b.ptr.value for b in (dbuf, sbuf, hbuf, mbuf, gbuf, out))
    V = ctypes.c_void_p
    p = lambda v: V(v) if v else None      # noqa: E731

    def gram(dict_=d, stride=9, nrec_=nrec, A_=A, astride=3, nouter=1, ninner=3, hout=h, mout=k):
        return lib.epgx_signal_component_gram(ctx.handle, p(dict_), stride, nrec_, A_, astride, nouter, ninner, p(hout), p(mout))

    def solve(dict_=d, stride=9, nrec_=nrec, A_=A, astride=3, nouter=1, ninner=3, H=h, mask=k, sig=s, sstride=nmeas, nmeas_=nmeas,
              reg=1e-8, tol=1e-10, group=0, w=o, g=o + 8 * A * nmeas, r=o + 8 * (A + 1) * nmeas, st=o + 8 * (A + 2) * nmeas):
        return lib.epgx_signal_nnls(ctx.handle, p(dict_), stride, nrec_, A_, astride, nouter, ninner, p(H), p(mask), p(sig), sstride,
                                    nmeas_, reg, tol, p(group), p(w), p(g), p(r), p(st))

    assert gram() == 0 and solve() == 0
    ctx.synchronize()
    good = out.download(np.float64, ((A + 3) * nmeas,)).copy()
    big = 1 << 62
    shared = [dict(dict_=0), dict(dict_=d + 8), dict(A_=0), dict(A_=65), dict(A_=-1), dict(nrec_=0), dict(nrec_=-2), dict(nouter=0),
              dict(ninner=0), dict(astride=-3), dict(astride=2), dict(stride=8), dict(stride=-9), dict(stride=big, nrec_=2 ** 31 - 1),
              dict(nouter=big, ninner=4), dict(nouter=2)]
    for kw in shared + [dict(hout=0), dict(mout=0), dict(hout=h + 4), dict(mout=k + 4)]:
        assert gram(**kw) == -1, kw
        assert b"epgx_signal_component_gram" in lib.epgx_last_error()
    mine = [dict(H=0), dict(mask=0), dict(sig=0), dict(w=0), dict(g=0), dict(r=0), dict(st=0), dict(sig=s + 8), dict(H=h + 4),
            dict(mask=k + 4), dict(group=gr + 4), dict(w=o + 4), dict(st=o + 8 * (A + 2) * nmeas + 2), dict(nmeas_=-1),
            dict(sstride=nmeas - 1), dict(sstride=-1), dict(sstride=big, nrec_=2 ** 31 - 1), dict(nmeas_=2 ** 31, sstride=2 ** 31),
            dict(reg=-1e-9), dict(reg=np.nan), dict(reg=np.inf), dict(tol=-1.0), dict(tol=np.nan), dict(tol=np.inf)]
    for kw in shared + mine:
        assert solve(**kw) == -1, kw
        assert b"epgx_signal_nnls" in lib.epgx_last_error()
    assert solve(nmeas_=0) == 0 and solve(nmeas_=0, sstride=0) == 0          # nothing to do
    ctx.synchronize()
    assert out.download(np.float64, ((A + 3) * nmeas,)).tobytes() == good.tobytes()      # the refused calls wrote nothing
    assert solve(group=gr, reg=0.0, tol=0.0) == 0
    ctx.synchronize()
    for b in (dbuf, sbuf, hbuf, mbuf, gbuf, out):
        b.free()


def cpmg(epg, t2, b1, necho=8):
    rlx = epg.E(5.0, 1000.0, t2)
    return [epg.T(90, 90)] + [epg.S(1), rlx, epg.T(160.0 * b1, 0), epg.S(1), rlx, epg.ADC] * necho


def test_end_to_end_from_the_simulator(ctx):
    """8-echo CPMG dictionary over 5 T2 x 3 B1 left on the device; one two-pool voxel per B1: the B1 is recovered and the
    short-T2 fraction is that of the references within the margin of the weights"""
    from epgpy_amd import epg, match, functions
    T2 = np.array([10.0, 20.0, 40.0, 80.0, 160.0])
    B1 = np.array([0.8, 0.9, 1.0])
    handle = epg.simulate(cpmg(epg, T2[:, None], B1[None, :]), out="device")
    if isinstance(handle, (tuple, list)):
        handle = handle[0]
    assert isinstance(handle, functions.DeviceSignal) and handle.shape == (8, 5, 3)
    D = np.asarray(handle)
    rng = np.random.default_rng(3)
    S = np.stack([0.25 * D[:, 1, j] + 0.75 * D[:, 3, j] for j in range(3)], axis=1)
    S = S + 0.002 * np.abs(S).max() * (rng.standard_normal(S.shape) + 1j * rng.standard_normal(S.shape))
    comp = match.Components(handle, 0)
    assert comp.groups == (3,) and comp.ncomp == 5
    res = match.nnls(comp, S)
    ref = match.nnls_host(D, S, 0)
    assert res.group.tolist() == [0, 1, 2] == ref.group.tolist() and (res.status == 0).all()
    assert res.unravel()[0].tolist() == [0, 1, 2]
    y = nc.Yardstick(D, S, 0, match.NNLS_REG)
    cond = nc.cond_ridge(D, 0, match.NNLS_REG)
    for m in range(3):
        sp = scipy_one(y, m, m, match.NNLS_REG)
        assert y.J(m, m, res.weights[:, m]) <= y.J(m, m, sp) * (1 + nc.MARGIN)
        assert y.J(m, m, res.weights[:, m]) <= y.J(m, m, ref.weights[:, m]) * (1 + nc.MARGIN)
        # the fraction is a quotient of sums of the weights: within the bound on the weights, over their sum
        bound = 5 * 2 * nc.weight_tol(cond[m], sp) / sp.sum()
        frac = match.NnlsResult(sp[:, None], np.array([m]), None, None, (3,)).fraction(0.0, 30.0, T2)[0]
        assert abs(res.fraction(0.0, 30.0, T2)[m] - frac) <= bound
        assert abs(res.fraction(0.0, 30.0, T2)[m] - ref.fraction(0.0, 30.0, T2)[m]) <= bound
    assert np.asarray(handle).tobytes() == D.tobytes()

"""GPU: the chi^2-driven ridge of epgpy_amd.match.nnls(..., chi2=) (nnls_kernel followed by nnls_chi2_kernel of
csrc/epgx_nnls_chi2.hip through epgx_signal_nnls_chi2), through the public entry, against the extended-precision quantities of
tests/nnls_chi2_cases.py: every sum in numpy.longdouble from the raw records, no Gram matrix.  tests/test_nnls_chi2_host.py shows
on the CPU that every voxel of every regular case reaches status 0 by the definition and by scipy inside brentq, so no status-0
exception is allowed here."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import nnls_cases as nc
from tests import nnls_chi2_cases as cc

pytestmark = pytest.mark.gpu

CASES = cc.cases()
_DEV = {}
NEW = ("mu", "chi2", "evals")


@pytest.fixture(scope="module")
def ctx():
    from epgpy_amd import _lib
    return _lib.get_context()


def device(name):
    """(Components, plain fit, regularised fit) of a case, computed once"""
    from epgpy_amd import match
    if name not in _DEV:
        c = CASES[name]
        comp = match.Components(c["D"], c["axis"])
        _DEV[name] = (comp, match.nnls(comp, c["S"], reg=c["reg"]), match.nnls(comp, c["S"], reg=c["reg"], chi2=c["chi2"]))
    return _DEV[name]


def fields(res, cols=slice(None)):
    out = [np.ascontiguousarray(res.weights.reshape(res.weights.shape[0], -1)[:, cols])]
    names = ("group", "residual", "status") + (NEW if res.mu is not None else ())
    return out + [np.ascontiguousarray(getattr(res, f).reshape(-1)[cols]) for f in names]


def same_bits(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes()


@pytest.mark.parametrize("name", sorted(CASES))
def test_case_against_yardstick(name):
    """1. the chi^2 condition, 2. optimality at the returned ridge against scipy and nnls_host, 3. the structure"""
    from epgpy_amd import match
    c = CASES[name]
    comp, plain, res = device(name)
    ref = match.nnls_host(c["D"], c["S"], c["axis"], reg=c["reg"], chi2=c["chi2"])
    y = nc.Yardstick(c["D"], c["S"], c["axis"], c["reg"])
    nmeas, chi2 = c["S"].shape[1], c["chi2"]
    assert res.weights.shape == (y.A, nmeas) and res.mu.shape == res.chi2.shape == res.evals.shape == (nmeas,)
    assert res.mu.dtype == np.float64 and res.chi2.dtype == np.float64 and res.evals.dtype == np.int32 and res.status.dtype == np.int32
    assert (plain.status == 0).all() and (res.status == 0).all() and (ref.status == 0).all()
    assert (res.weights >= 0).all()
    assert res.group.tobytes() == plain.group.tobytes()
    assert (res.evals <= cc.EVALS).all() and (res.evals >= 0).all()
    worst = 0.0
    for m in range(nmeas):
        g = int(res.group[m])
        E = y.energy(m)
        x0, x = plain.weights[:, m], res.weights[:, m]
        Jd0, Jd = cc.misfit(y, m, g, x0), cc.misfit(y, m, g, x)
        slack = 2 * cc.gram_rounding(y.nrec, y.A, E) / float(Jd0)
        got = abs(float(Jd / Jd0) - chi2) / chi2
        worst = max(worst, got)
        assert got <= cc.RTOL + slack, (name, m, got)
        assert abs(res.chi2[m] - float(Jd / Jd0)) <= chi2 * slack
        assert abs(res.residual[m] - float(np.sqrt(Jd))) <= nc.residual_tol(y.nrec, y.A, E)
        assert res.mu[m] >= float(y.mu[g]) * (1 - 2.0 ** -50)      # (mu_0 in float64 against the yardstick's longdouble)
        assert (x ** 2).sum() <= (x0 ** 2).sum() * (1 + nc.MARGIN)
        Jx = cc.objective(y, m, g, x, res.mu[m])
        assert Jx <= cc.objective(y, m, g, cc.scipy_at(y, m, g, res.mu[m]), res.mu[m]) * (1 + nc.MARGIN), (name, m)
        # nnls_host's weights are those of ITS ridge, a rounding of exp and log away: the device's weights at the device's ridge
        # against the definition's fit at that same ridge
        H = (np.conj(y.D[:, :, g]).T @ y.D[:, :, g]).real
        f = (np.conj(y.D[:, :, g]).T @ y.S[:, m]).real
        xh = match._nnls_task(H, y.valid[:, g], float(res.mu[m]), f, E, match.NNLS_TOL)[0]
        assert Jx <= cc.objective(y, m, g, xh, res.mu[m]) * (1 + nc.MARGIN), (name, m, "nnls_host")
        assert Jx <= cc.objective(y, m, g, ref.weights[:, m], res.mu[m]) * (1 + nc.MARGIN), (name, m, "nnls_host at its own ridge")
    print(name, "largest |Jd/Jd0 - chi2|/chi2:", worst, "evals max", res.evals.max(), "mean", res.evals.mean())
    if c["decay"] and y.A > 1:      # (one atom: the passive set cannot grow)
        assert ((res.weights > 0).sum(axis=0) > (plain.weights > 0).sum(axis=0)).any(), "a search that never moves"


@pytest.mark.parametrize("name", ["a33_r33_g3_m65", "a64_r33_g3_m9"])
def test_chi2_none_returns_todays_bytes(name):
    from epgpy_amd import match
    c = CASES[name]
    comp, plain, _ = device(name)
    again = match.nnls(comp, c["S"], reg=c["reg"], chi2=None)
    assert again.mu is None and again.chi2 is None and again.evals is None
    same_bits(fields(again), fields(plain))
    fixed = match.nnls(comp, c["S"], reg=c["reg"], group=plain.group, chi2=None, chi2_rtol=0.5)
    same_bits(fields(fixed), fields(plain))


@pytest.mark.parametrize("name", ["a33_r33_g3_m65", "a64_r33_g3_m9", "axis_middle"])
def test_a_voxel_does_not_depend_on_the_others(name):
    """a voxel alone, in the permuted call, in the full call and with its group fixed: the same bytes in every field"""
    from epgpy_amd import match
    c = CASES[name]
    comp, plain, full = device(name)
    nmeas = c["S"].shape[1]
    kw = dict(reg=c["reg"], chi2=c["chi2"])
    perm = np.random.default_rng(5).permutation(nmeas)
    same_bits(fields(match.nnls(comp, np.ascontiguousarray(c["S"][:, perm]), **kw)), fields(full, perm))
    for m in (0, nmeas // 2, nmeas - 1):
        one = match.nnls(comp, c["S"][:, m], **kw)
        assert one.mu.shape == () and one.weights.shape == (comp.ncomp,)
        same_bits(fields(one), fields(full, slice(m, m + 1)))
    same_bits(fields(match.nnls(comp, c["S"], group=full.group, **kw)), fields(full))
    # the old fields of the baseline inside the new kernel are those of nnls_kernel: a cap of 0 fits returns them
    base = match.nnls(comp, c["S"], _max_evals=0, **kw)
    assert (base.status == 3).all() and (base.evals == 0).all() and (base.chi2 == 1).all()
    same_bits(fields(base)[:3], fields(plain)[:3])


def test_statuses_3_and_4_and_degenerates():
    from epgpy_amd import match
    e = cc.edge()
    comp = match.Components(e["D"], 0)
    plain = match.nnls(comp, e["S"], reg=e["reg"])
    res = match.nnls(comp, e["S"], reg=e["reg"], chi2=e["chi2"])
    ref = match.nnls_host(e["D"], e["S"], 0, reg=e["reg"], chi2=e["chi2"])
    assert res.status.tolist() == ref.status.tolist() == [4, 3, 3, 0, 4]
    rest = [0, 1, 2, 4]
    same_bits(fields(res, rest)[:3], fields(plain, rest)[:3])
    assert (res.chi2[rest] == 1).all() and (res.evals[rest] == 0).all() and np.allclose(res.mu[rest], ref.mu[rest], rtol=1e-14, atol=0)
    assert (res.weights[:, 4] == 0).all() and res.residual[4] == 0                        # the all-zero signal
    assert res.evals[3] > 0 and ref.evals[3] > 0 and abs(res.chi2[3] / e["chi2"] - 1) <= cc.RTOL
    for cap in (0, 1, int(res.evals[3]) - 1):                                             # status 3 by the cap
        low = match.nnls(comp, e["S"][:, 3], reg=e["reg"], chi2=e["chi2"], _max_evals=cap)
        assert low.status == 3 and low.evals == cap and (low.weights >= 0).all()
        assert 1 <= low.chi2 < e["chi2"] * (1 - cc.RTOL) and low.mu >= res.mu[0]
    assert match.nnls(comp, e["S"][:, 3], reg=e["reg"], chi2=e["chi2"], _max_evals=int(res.evals[3])).status == 0

    c = nc.special()                                                                      # NaN and all-zero atoms, an invalid group
    D, S = c["D"], c["S"]
    comp = match.Components(D, 0)
    plain = match.nnls(comp, S, reg=c["reg"])
    res = match.nnls(comp, S, reg=c["reg"], chi2=1.02)
    assert res.group.tolist() == plain.group.tolist() == [0, 1, 1, 1, 0, 0, 0]
    assert res.status[0] == 4 and (res.status[1:] == 0).all() and np.isfinite(res.weights).all() and (res.weights >= 0).all()
    assert (res.weights[[2, 4], 1:4] == 0).all()
    fixed = match.nnls(comp, S, reg=c["reg"], chi2=1.02, group=np.array([3, 1, 1, 0, 3, 0, 2]))
    assert (fixed.weights[:, 6] == 0).all() and fixed.status[6] == 3 and fixed.evals[6] == 0      # no valid atom: x = 0, Jd = E
    same_bits(fields(fixed, [1, 2, 5]), fields(res, [1, 2, 5]))
    out = match.nnls(comp, S, reg=c["reg"], chi2=1.02, group=np.array([-1, 4, 0, 0, 0, 0, 2 ** 40]))
    bad = [0, 1, 6]
    assert out.group[bad].tolist() == [-1, -1, -1] and np.isnan(out.weights[:, bad]).all() and np.isnan(out.residual[bad]).all()
    assert (out.status[bad] == 2).all() and np.isnan(out.mu[bad]).all() and np.isnan(out.chi2[bad]).all() and (out.evals[bad] == 0).all()
    same_bits(fields(out, [4, 5]), fields(res, [4, 5]))
    nonfinite = S.copy()
    nonfinite[3, 2] = np.nan
    nonfinite[0, 5] = np.inf
    out = match.nnls(comp, nonfinite, reg=c["reg"], chi2=1.02)
    assert out.group[[2, 5]].tolist() == [-1, -1] and (out.status[[2, 5]] == 2).all() and np.isnan(out.weights[:, [2, 5]]).all()
    same_bits(fields(out, [1, 3, 4, 6]), fields(res, [1, 3, 4, 6]))
    for kw in (dict(chi2=1.0), dict(chi2=np.inf), dict(chi2=np.nan), dict(chi2=[1.02])):
        with pytest.raises(ValueError, match="chi2"):
            match.nnls(comp, S, **kw)
    for bad in (0.0, 1.0, np.nan):
        with pytest.raises(ValueError, match="chi2_rtol"):
            match.nnls(comp, S, chi2=1.02, chi2_rtol=bad)
    with pytest.raises(ValueError, match="reg"):
        match.nnls(comp, S, chi2=1.02, reg=0.0)


def test_handles(ctx):
    """a strided DeviceSignal and a DeviceJacobian as the dictionary, a DeviceSignal as the signals: the bytes of the plain arrays"""
    from epgpy_amd import match, functions, _lib
    c = CASES["axis_last"]
    D, S = c["D"], c["S"]
    _, _, want = device("axis_last")
    kw = dict(reg=c["reg"], chi2=c["chi2"])
    nrec, grid, nvox = D.shape[0], D.shape[1:], int(np.prod(D.shape[1:]))
    hostbuf = np.full((nrec * 3, nvox), np.nan + 1j * np.nan, dtype=np.complex128)
    hostbuf[1::3] = D.reshape(nrec, nvox)
    buf = _lib.DeviceBuffer(ctx, hostbuf.nbytes)
    buf.upload(hostbuf)
    sig = functions.DeviceSignal(buf, nrec * 3, grid, 1, 3)
    same_bits(fields(match.nnls(match.Components(sig, 2), S, **kw)), fields(want))
    jac = functions.DeviceJacobian(buf, nrec, grid, 1, 3, 0, [1, 2], ["x", "y"])
    hostbuf[0::3] = D.reshape(nrec, nvox)
    hostbuf[1::3] = np.nan
    buf.upload(hostbuf)
    sbuf = _lib.DeviceBuffer(ctx, S.nbytes)
    sbuf.upload(S)
    dsig = functions.DeviceSignal(sbuf, nrec, (S.shape[1],), 0, 1)
    same_bits(fields(match.nnls(match.Components(jac, -1), dsig, **kw)), fields(want))
    buf.free()


def test_entry_point_errors(ctx):
    """every EPGX_ERR_INVALID condition of epgx_signal_nnls_chi2 through raw calls: -1, a message that names the entry, nothing written"""
    from epgpy_amd import _lib
    lib = ctx.lib
    c = nc.cases()["a3_r8_g3_m65"]
    D, S = c["D"].reshape(8, 9), c["S"]
    nrec, A, G, nmeas = 8, 3, 3, 65
    dbuf, sbuf = _lib.DeviceBuffer(ctx, D.nbytes), _lib.DeviceBuffer(ctx, S.nbytes)
    dbuf.upload(D)
    sbuf.upload(S)
    hbuf, mbuf = _lib.DeviceBuffer(ctx, 8 * G * A * A, itemsize=8), _lib.DeviceBuffer(ctx, 8 * G, itemsize=8)
    gbuf = _lib.DeviceBuffer(ctx, 8 * nmeas, itemsize=8)
    gbuf.upload(np.zeros(nmeas, dtype=np.int64))
    out = _lib.DeviceBuffer(ctx, 8 * (A + 6) * nmeas, itemsize=8)
    d, s, h, k, gr, o = (b.ptr.value for b in (dbuf, sbuf, hbuf, mbuf, gbuf, out))
    V = ctypes.c_void_p
    p = lambda v: V(v) if v else None      # noqa: E731
    row = lambda i: o + 8 * (A + i) * nmeas      # noqa: E731
    assert lib.epgx_signal_component_gram(ctx.handle, p(d), 9, nrec, A, 3, 1, 3, p(h), p(k)) == 0

    def solve(dict_=d, stride=9, nrec_=nrec, A_=A, astride=3, nouter=1, ninner=3, H=h, mask=k, sig=s, sstride=nmeas, nmeas_=nmeas,
              reg=1e-8, tol=1e-10, group=0, chi2=1.02, rtol=1e-3, evals=cc.EVALS, w=o, g=row(0), r=row(1), st=row(2), mu=row(3),
              ratio=row(4), ev=row(5)):
        return lib.epgx_signal_nnls_chi2(ctx.handle, p(dict_), stride, nrec_, A_, astride, nouter, ninner, p(H), p(mask), p(sig), sstride,
                                         nmeas_, reg, tol, p(group), chi2, rtol, evals, p(w), p(g), p(r), p(st), p(mu), p(ratio), p(ev))

    assert solve() == 0
    ctx.synchronize()
    good = out.download(np.float64, ((A + 6) * nmeas,)).copy()
    big = 1 << 62
    bad = [dict(dict_=0), dict(dict_=d + 8), dict(A_=0), dict(A_=65), dict(A_=-1), dict(nrec_=0), dict(nrec_=-2), dict(nouter=0),
           dict(ninner=0), dict(astride=-3), dict(astride=2), dict(stride=8), dict(stride=-9), dict(stride=big, nrec_=2 ** 31 - 1),
           dict(nouter=big, ninner=4), dict(nouter=2),
           dict(H=0), dict(mask=0), dict(sig=0), dict(w=0), dict(g=0), dict(r=0), dict(st=0), dict(mu=0), dict(ratio=0), dict(ev=0),
           dict(sig=s + 8), dict(H=h + 4), dict(mask=k + 4), dict(group=gr + 4), dict(w=o + 4), dict(st=row(2) + 2), dict(mu=row(3) + 4),
           dict(ratio=row(4) + 4), dict(ev=row(5) + 2), dict(nmeas_=-1), dict(sstride=nmeas - 1), dict(sstride=-1),
           dict(sstride=big, nrec_=2 ** 31 - 1), dict(nmeas_=2 ** 31, sstride=2 ** 31),
           dict(reg=-1e-9), dict(reg=np.nan), dict(reg=np.inf), dict(reg=0.0), dict(tol=-1.0), dict(tol=np.nan), dict(tol=np.inf),
           dict(chi2=1.0), dict(chi2=0.0), dict(chi2=np.nan), dict(chi2=np.inf), dict(rtol=0.0), dict(rtol=1.0), dict(rtol=np.nan),
           dict(evals=-1), dict(evals=cc.EVALS + 1)]
    for kw in bad:
        assert solve(**kw) == -1, kw
        assert b"epgx_signal_nnls_chi2" in lib.epgx_last_error()
    assert solve(nmeas_=0) == 0 and solve(nmeas_=0, sstride=0) == 0          # nothing to do
    ctx.synchronize()
    assert out.download(np.float64, ((A + 6) * nmeas,)).tobytes() == good.tobytes()      # the refused calls wrote nothing
    assert solve(group=gr) == 0
    ctx.synchronize()
    for b in (dbuf, sbuf, hbuf, mbuf, gbuf, out):
        b.free()


def test_symbols(ctx):
    """the entry and its 26 arguments in the public header and in the library, at ABI 11"""
    from epgpy_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "epgx.h")) as fh:
        text = fh.read()
    proto = re.search(r"int epgx_signal_nnls_chi2\(([^;]*)\);", text)
    assert proto and len(proto.group(1).split(",")) == 26
    assert re.search(r"#define\s+EPGX_ABI_VERSION\s+11\b", text)
    assert hasattr(ctx.lib, "epgx_signal_nnls_chi2") and ctx.lib.epgx_abi_version() == 11
    assert len(_lib.SYMBOLS["epgx_signal_nnls_chi2"][1]) == 26


def cpmg(epg, t2, b1, necho=8):
    rlx = epg.E(5.0, 1000.0, t2)
    return [epg.T(90, 90)] + [epg.S(1), rlx, epg.T(160.0 * b1, 0), epg.S(1), rlx, epg.ADC] * necho


def test_end_to_end_from_the_simulator():
    """8-echo CPMG dictionary over 5 T2 x 3 B1 left on the device: the B1 of the plain fit, the chi^2 condition, a spectrum at
    least as wide"""
    from epgpy_amd import epg, match
    T2 = np.array([10.0, 20.0, 40.0, 80.0, 160.0])
    B1 = np.array([0.8, 0.9, 1.0])
    handle = epg.simulate(cpmg(epg, T2[:, None], B1[None, :]), out="device")
    if isinstance(handle, (tuple, list)):
        handle = handle[0]
    D = np.asarray(handle)
    rng = np.random.default_rng(3)
    S = np.stack([0.25 * D[:, 1, j] + 0.75 * D[:, 3, j] for j in range(3)], axis=1)
    S = S + 0.02 * np.abs(S).max() * (rng.standard_normal(S.shape) + 1j * rng.standard_normal(S.shape))
    comp = match.Components(handle, 0)
    plain = match.nnls(comp, S)
    res = match.nnls(comp, S, chi2=1.02)
    assert res.group.tolist() == plain.group.tolist() == [0, 1, 2] and (res.status == 0).all()
    y = nc.Yardstick(D, S, 0, match.NNLS_REG)
    for m in range(3):
        Jd0, Jd = cc.misfit(y, m, m, plain.weights[:, m]), cc.misfit(y, m, m, res.weights[:, m])
        assert abs(float(Jd / Jd0) - 1.02) / 1.02 <= cc.RTOL + 2 * cc.gram_rounding(8, 5, y.energy(m)) / float(Jd0)
        assert (res.weights[:, m] > 0).sum() >= (plain.weights[:, m] > 0).sum()
    assert np.isfinite(res.gmean(T2)).all() and np.all((res.fraction(0.0, 30.0, T2) >= 0) & (res.fraction(0.0, 30.0, T2) <= 1))

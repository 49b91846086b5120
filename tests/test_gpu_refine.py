"""GPU: epgpy_amd.match.refine (refine_kernel of csrc/epgx_refine.hip through epgx_signal_refine) against the extended-precision
yardstick of tests/refine_cases.py, whose bounds are derived there and not measured.  Shapes sit around the 64-voxel wavefront
and on both sides of the slice boundaries 16 | 17, 32 | 33, 64 | 65 records; tests/test_refine_host.py shows on the CPU that at
least 90 % of the voxels of every case are decisive and that the residual bounds are not vacuous."""
import ctypes

import numpy as np
import pytest

from tests import refine_cases as rc

pytestmark = pytest.mark.gpu

CASES = rc.cases()
_YARD = {}


def yard(name):
    if name not in _YARD:
        _YARD[name] = rc.yardstick(CASES[name])
    return _YARD[name]


@pytest.fixture(scope="module")
def ctx():
    from epgpy_amd import _lib
    return _lib.get_context()


def run(case, **kw):
    from epgpy_amd import match
    kw.setdefault("variables", case.get("rows"))
    return match.refine(case["D"], case["S"], case["index"], jacobian=case["J"], **kw)


def same_bits(got, want):
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes()


@pytest.mark.parametrize("name", sorted(CASES))
def test_case_against_yardstick(name):
    """every case through match.refine on host arrays"""
    case = CASES[name]
    free = run(case)
    P = yard(name).P
    assert free.delta.shape == (case["S"].shape[1], P) and free.scale.shape == free.score.shape == (case["S"].shape[1],)
    assert free.variables == list(case.get("rows", range(P)))
    if "limit" in case:
        got = run(case, limit=case["limit"])
        resolved = np.isfinite(free.delta).all(axis=1)
        clipped = np.any(got.delta != free.delta, axis=1) & resolved
        assert clipped.any() and (~clipped & resolved).any()
        worst = yard(name).check(got.delta, got.scale, got.score, unclipped=free.delta, limit=case["limit"], what=name)
    else:
        worst = yard(name).check(free.delta, free.scale, free.score, what=name)
    print(name, "largest share of the bounds used:", worst)


def padded_jacobian(ctx, D, J, rows, nrow, pad, lead):
    """[record][row][atom] in a device buffer: row 0 the dictionary, column p of J at row rows[p], rows of natoms + pad elements,
    `lead` elements in; every other row, the padding and the lead hold NaN (a kernel that read them would show it)"""
    from epgpy_amd import _lib
    nrec, natoms = D.shape
    stride = natoms + pad
    host = np.full(lead + nrec * nrow * stride, np.nan + 1j * np.nan, dtype=np.complex128)
    block = host[lead:].reshape(nrec, nrow, stride)
    block[:, 0, :natoms] = D
    for p, r in enumerate(rows):
        block[:, r, :natoms] = J[:, :, p]
    buf = _lib.DeviceBuffer(ctx, host.nbytes)
    buf.upload(host)
    return buf, buf.ptr.value + 16 * lead, nrow * stride, stride


def padded(ctx, A, pad, lead=0):
    from epgpy_amd import _lib
    nrec, ncol = A.shape
    host = np.full(lead + nrec * (ncol + pad), np.nan + 1j * np.nan, dtype=np.complex128)
    host[lead:].reshape(nrec, ncol + pad)[:, :ncol] = A
    buf = _lib.DeviceBuffer(ctx, host.nbytes)
    buf.upload(host)
    return buf, buf.ptr.value + 16 * lead, ncol + pad


@pytest.mark.parametrize("name", ["gauss_257_131_37_p3", "gauss_17_65_33_p4", "special"])
def test_raw_entry_on_padded_buffers(ctx, name):
    """through _lib.signal_refine: NaN padding, a lead, the Jacobian's columns at scattered rows among NaN rows"""
    from epgpy_amd import _lib
    case = CASES[name]
    D, J, S, idx = case["D"], case["J"], case["S"], case["index"]
    P = J.shape[2]
    dense = run(case)
    rows = [5, 2, 6, 3][:P]
    jbuf, jptr, rstride, stride = padded_jacobian(ctx, D, J, rows, 7, pad=3, lead=7)
    sbuf, sptr, sstride = padded(ctx, S, 5, lead=3)
    try:
        delta, scale, score = _lib.signal_refine(ctx, jptr, rstride, stride, 7, D.shape[0], rows, D.shape[1], sptr, sstride, S.shape[1], idx)
    finally:
        jbuf.free()
        sbuf.free()
    same_bits((np.ascontiguousarray(delta.T), scale, score), (dense.delta, dense.scale, dense.score))
    yard(name).check(delta.T.copy(), scale, score, what=name)


@pytest.mark.parametrize("name", ["gauss_257_131_37_p3", "gauss_17_65_1000_p4", "decay_257_63_65_p3", "gauss_17_131_16_p4", "special"])
def test_a_voxel_does_not_depend_on_the_others(name):
    """a voxel refined alone, in a permuted call and in the full call gives the same bytes"""
    case = CASES[name]
    full = run(case)
    nmeas = case["S"].shape[1]
    perm = np.random.default_rng(5).permutation(nmeas)
    mixed = run(dict(case, S=np.ascontiguousarray(case["S"][:, perm]), index=case["index"][perm]))
    same_bits((mixed.delta, mixed.scale, mixed.score), (full.delta[perm], full.scale[perm], full.score[perm]))
    for m in (0, nmeas // 2, nmeas - 1):
        one = run(dict(case, S=case["S"][:, m], index=case["index"][m]))
        assert one.scale.shape == () and one.delta.shape == (full.delta.shape[1],)
        same_bits((one.delta.reshape(1, -1), one.scale.reshape(1), one.score.reshape(1)),
                  (full.delta[m:m + 1], full.scale[m:m + 1], full.score[m:m + 1]))


def test_index_outside_the_atoms_straight_to_the_library(ctx):
    """indices that match.refine refuses, handed to _lib.signal_refine: the voxels come back NaN with scale 0 and score 0, and
    their neighbours keep their bits.  (The kernel loads nothing for them; the NaN rows around the atoms would show a read.)"""
    from epgpy_amd import _lib
    case = CASES["gauss_17_65_33_p4"]
    D, J, S, idx = case["D"], case["J"], case["S"], case["index"].copy()
    dense = run(case)
    bad = [0, 7, 63, 64]
    idx[bad] = [17, -2, 2 ** 40, -2 ** 62]
    rows = [1, 2, 3, 4]
    jbuf, jptr, rstride, stride = padded_jacobian(ctx, D, J, rows, 5, pad=1, lead=1)
    sbuf, sptr, sstride = padded(ctx, S, 0)
    try:
        delta, scale, score = _lib.signal_refine(ctx, jptr, rstride, stride, 5, D.shape[0], rows, 17, sptr, sstride, S.shape[1], idx)
    finally:
        jbuf.free()
        sbuf.free()
    assert np.isnan(delta[:, bad]).all() and (scale[bad] == 0).all() and (score[bad] == 0).all()
    keep = np.setdiff1d(np.arange(S.shape[1]), bad)
    same_bits((np.ascontiguousarray(delta.T[keep]), scale[keep], score[keep]), (dense.delta[keep], dense.scale[keep], dense.score[keep]))


def test_shapes_and_empty(ctx):
    from epgpy_amd import match
    D, J, S, idx = rc.gaussian_case(6, 12, 6, 5, 2)
    res = match.refine(D.reshape(5, 3, 4), S.reshape(5, 2, 3), idx.reshape(2, 3), jacobian=J.reshape(5, 3, 4, 2), limit=0.5)
    assert res.delta.shape == (2, 3, 2) and res.scale.shape == (2, 3) and res.grid == (3, 4) and res.index.dtype == np.int64
    rc.Yardstick(D, J, S, idx).check(res.delta.reshape(6, 2), res.scale, res.score)
    est = res.estimate([np.arange(3.0)[:, None], np.arange(4.0)[None, :]])
    assert est.shape == (2, 3, 2) and np.isfinite(est).all()
    real = match.refine(D, np.ascontiguousarray(S.real), idx, jacobian=J)
    rc.Yardstick(D, J, S.real.astype(np.complex128), idx).check(real.delta, real.scale, real.score)
    empty = match.refine(D, np.zeros((5, 0)), np.zeros(0, dtype=np.int64), jacobian=J)
    assert empty.delta.shape == (0, 2) and empty.score.shape == (0,)


def mse_train(epg, t2, b1, necho=8, **kw):
    rlx = epg.E(5.0, 1000.0, t2, **kw)
    return [epg.T(90, 90)] + [epg.S(1), rlx, epg.T(150.0 * b1, 0), epg.S(1), rlx, epg.ADC] * necho


def test_end_to_end_from_the_simulator(ctx):
    """8-echo multi-spin-echo dictionary over 33 T2 x 3 B1 values with its T2 derivative left on the device; signals simulated at
    off-grid T2; match, then refine straight from the handle"""
    from epgpy_amd import epg, match, functions
    T2 = np.geomspace(30.0, 200.0, 33)[:, None]
    B1 = np.array([0.8, 0.9, 1.0])[None, :]
    jac = epg.simulate(mse_train(epg, T2, B1, order1=["T2"]), probe=epg.Jacobian(["magnitude", "T2"]), out="device")
    if isinstance(jac, (tuple, list)):
        jac = jac[0]
    assert isinstance(jac, functions.DeviceJacobian) and jac.shape == (8, 33, 3, 2)
    before = np.asarray(jac)

    rng = np.random.default_rng(23)
    at = rng.integers(1, 32, 40)
    step = np.log(T2[1, 0] / T2[0, 0])
    truth = T2[at, 0] * np.exp(rng.uniform(0.1, 0.45, 40) * rng.choice([-1.0, 1.0], 40) * step)
    b1 = B1[0, rng.integers(0, 3, 40)]
    pd = (0.5 + rng.random(40)) * np.exp(2j * np.pi * rng.random(40))
    S = np.asarray(epg.simulate(mse_train(epg, truth, b1))).reshape(8, 40) * pd

    dic = match.Dictionary(jac)
    assert dic.jacobian is jac
    res = match.match(dic, S)
    ref = match.refine(jac, S, res, variables=["T2"])
    assert ref.variables == ["T2"] and ref.grid == (33, 3) and ref.delta.shape == (40, 1)
    same_bits((match.refine(dic, S, res.index, variables=["T2"]).delta,), (ref.delta,))

    D, J = before[..., 0].reshape(8, 99), before[..., 1].reshape(8, 99, 1)
    y = rc.Yardstick(D, J, S, res.index)
    worst = y.check(ref.delta, ref.scale, ref.score, what="mse")
    print("mse", worst)
    assert y.must_resolve.all()
    host = match.refine_host(D, J, S, res.index)
    y.check(host.delta, host.scale, host.score, what="mse host")
    same_bits((match.refine(D, S, res.index, jacobian=J).delta,), (ref.delta,))

    est = ref.estimate([T2])[:, 0]
    grid = np.broadcast_to(T2, (33, 3)).reshape(-1)[res.index]
    assert np.all(np.abs(est - truth) < np.abs(grid - truth)), np.max(np.abs(est - truth) / np.abs(grid - truth))
    assert np.all(ref.score >= res.score - 1e-12)

    auto = match.refine(jac, S, res, limit=[50.0])          # "magnitude" is the state itself: left out by default, refused by name
    assert auto.variables == ["T2"]
    same_bits((auto.delta, auto.scale, auto.score), (ref.delta, ref.scale, ref.score))
    with pytest.raises(ValueError, match="probed state"):
        match.refine(jac, S, res, variables=["magnitude", "T2"])
    after = np.asarray(jac)
    assert after.tobytes() == before.tobytes()


def test_what_refine_does_not_take(ctx):
    from epgpy_amd import match, functions, _lib
    D, J, S, idx = rc.gaussian_case(5, 17, 9, 5, 2)
    dic = match.Dictionary(D)
    with pytest.raises(ValueError, match="DeviceJacobian"):
        match.refine(dic, S, idx)
    with pytest.raises(NotImplementedError, match="complex64"):
        match.refine(match.Dictionary(D, dtype=np.complex64), S, idx)
    basis = match.compress(dic, rank=3)
    with pytest.raises(NotImplementedError, match="compressed"):
        match.refine(basis.dictionary, S, idx)
    with pytest.raises(ValueError, match="derivative"):
        match.refine(dic.records, S, idx)
    sharded = object.__new__(functions.ShardedDeviceSignal)
    with pytest.raises(NotImplementedError, match="ShardedDeviceSignal"):
        match.refine(sharded, S, idx)
    hess = object.__new__(functions.DeviceHessian)
    with pytest.raises(NotImplementedError, match="DeviceHessian"):
        match.refine(hess, S, idx)
    host = np.stack([D] + [J[:, :, p] for p in range(2)], axis=1)
    buf = _lib.DeviceBuffer(ctx, host.nbytes)
    buf.upload(host)
    jac = functions.DeviceJacobian(buf, 5, (17,), 1, 3, 0, [1, 2], ["x", "y"])
    good = match.refine(jac, S, idx, variables=["y", "x"])
    rc.Yardstick(D, J[:, :, ::-1], S, idx).check(good.delta, good.scale, good.score)
    with pytest.raises(ValueError, match="not a column"):
        match.refine(jac, S, idx, variables=["z"])
    with pytest.raises(ValueError, match="jacobian="):
        match.refine(jac, S, idx, jacobian=J)
    buf.free()
    with pytest.raises(_lib.EpgxError):
        match.refine(jac, S, idx)


def test_entry_point_errors(ctx):
    """every EPGX_ERR_INVALID condition of include/epgx.h through raw calls: -1, a message, nothing launched"""
    from epgpy_amd import _lib
    lib = ctx.lib
    natoms, nmeas, nrec, P = 17, 9, 5, 2
    D, J, S, idx = rc.gaussian_case(5, natoms, nmeas, nrec, P)
    host = np.stack([D, J[:, :, 0], J[:, :, 1]], axis=1)
    jbuf, sbuf = _lib.DeviceBuffer(ctx, host.nbytes), _lib.DeviceBuffer(ctx, S.nbytes)
    jbuf.upload(host)
    sbuf.upload(S)
    ibuf = _lib.DeviceBuffer(ctx, 8 * nmeas, itemsize=8)
    ibuf.upload(idx)
    out = _lib.DeviceBuffer(ctx, (24 + 8 * P) * nmeas, itemsize=8)
    j, s, i, o = jbuf.ptr.value, sbuf.ptr.value, ibuf.ptr.value, out.ptr.value
    V = ctypes.c_void_p

    def call(jac=j, rstride=3 * natoms, stride=natoms, nrow=3, nrec_=nrec, rows=(1, 2), natoms_=natoms, sig=s, sstride=nmeas,
             nmeas_=nmeas, index=i, limit=None, rcond=1e-10, delta=o + 16 * nmeas, scale=o, score=o + (16 + 8 * P) * nmeas, nparam=None):
        p = lambda v: V(v) if v else None      # noqa: E731
        r = np.array(rows, dtype=np.int32) if rows is not None else None
        lim = np.array(limit, dtype=np.float64) if limit is not None else None
        return lib.epgx_signal_refine(ctx.handle, p(jac), rstride, stride, nrow, nrec_, len(rows) if nparam is None else nparam,
                                      r.ctypes.data if r is not None else None, natoms_, p(sig), sstride, nmeas_, p(index),
                                      lim.ctypes.data if lim is not None else None, rcond, p(delta), p(scale), p(score))

    assert call() == 0
    ctx.synchronize()
    good = out.download(np.float64, ((3 + P) * nmeas,)).copy()
    big = 1 << 62
    bad = [dict(jac=0), dict(rows=None, nparam=2), dict(sig=0), dict(index=0), dict(delta=0), dict(scale=0), dict(score=0),
           dict(jac=j + 8), dict(sig=s + 8), dict(scale=o + 8), dict(index=i + 4), dict(delta=o + 16 * nmeas + 4),
           dict(score=o + (16 + 8 * P) * nmeas + 4), dict(rows=()), dict(rows=(1, 2, 1, 2, 1), nrow=3), dict(nrec_=0), dict(nrec_=-3),
           dict(nrow=0), dict(natoms_=0), dict(nmeas_=-1), dict(stride=natoms - 1), dict(stride=0), dict(rstride=3 * natoms - 1),
           dict(rstride=big, nrec_=2 ** 31 - 1), dict(sstride=nmeas - 1), dict(sstride=big, nrec_=2 ** 31 - 1),
           dict(rows=(0, 1)), dict(rows=(1, 3)), dict(rows=(-1, 1)), dict(rows=(2, 2)), dict(limit=(1.0, 0.0)), dict(limit=(-1.0, 1.0)),
           dict(limit=(np.nan, 1.0)), dict(rcond=-1e-3), dict(rcond=1.0), dict(rcond=np.nan)]
    for kw in bad:
        assert call(**kw) == -1, kw
        assert b"epgx_signal_refine" in lib.epgx_last_error()
    assert call(nmeas_=0) == 0 and call(nmeas_=0, sstride=0) == 0          # nothing to do
    assert call(limit=(np.inf, 2.0), rcond=0.0) == 0
    ctx.synchronize()
    assert out.download(np.float64, ((3 + P) * nmeas,)).tobytes() == good.tobytes()      # the refused calls wrote nothing (inf, 2.0 clips nothing)
    for b in (jbuf, sbuf, ibuf, out):
        b.free()

"""GPU: stats.crlb / stats.crlb_split on a DeviceJacobian (crlb_kernel<P> through epgx_signal_crlb) against the same formula in
extended precision (tests/stats_cases.py: yardstick, tolerance max(64, nrec) * 2.2e-16 * cond2(I) per voxel, voxels with
cond2 > 1e8 excluded, at most 10 % of a case).

Shapes: the smallest at which the kernel can go wrong -- voxel counts around one wavefront and one block (1, 63, 64, 65, 257),
record counts around the unroll factor (4), the slice boundaries (64 / 65, 128 / 129, 256 / 257: 1 -> 2 -> 4 -> 8 wavefronts per
voxel) and P, P + 1; every P; a probe that is not the first of its record (record stride != nrow * nvox); permuted rows and
strict subsets of the rows."""
import ctypes

import numpy as np
import pytest

from tests import stats_cases as sc

pytestmark = pytest.mark.gpu

W4 = np.array([0.5, 2.0, 1.25, 3.0])


@pytest.fixture(scope="module")
def ctx():
    from epgpy_amd import _lib
    return _lib.get_context(0)


def check_case(ctx, records, j, rows, what):
    """crlb plain / W / sigma2 / log and crlb_split with and without W / log on one uploaded Jacobian"""
    from epgpy_amd import stats
    P = len(rows)
    jac = sc.upload_jacobian(ctx, records, j, rows)
    J = sc.columns(records, j, rows)
    y1, yq = sc.Yardstick(J), sc.Yardstick(J, sigma2=0.25)
    W = W4[:P]
    y1.check(stats.crlb(jac), y1.cost(), what=f"{what} crlb")
    y1.check(stats.crlb(jac, W=W), y1.cost(W), what=f"{what} crlb W")
    yq.check(stats.crlb(jac, sigma2=0.25), yq.cost(), what=f"{what} crlb sigma2")
    y1.check(stats.crlb(jac, log=True), y1.cost(), log=True, what=f"{what} crlb log")
    y1.check(stats.crlb_split(jac), y1.split(), what=f"{what} split")
    y1.check(stats.crlb_split(jac, W=W, log=True), y1.split(W), log=True, what=f"{what} split W log")
    assert stats.crlb(jac).shape == (records.shape[-1],) and stats.crlb_split(jac).shape == (P, records.shape[-1])


def record_counts(P):
    return sorted({n for n in (P, P + 1, 3, 4, 5, 7, 63, 64, 65, 128, 129, 256, 257) if n >= P})


@pytest.mark.parametrize("nvox", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("P", [1, 2, 3, 4])
def test_crlb_gaussian(ctx, P, nvox):
    """rows 0 .. P - 1 of probe 1 of 2 (record stride 2 * P * nvox)"""
    for nrec in record_counts(P):
        records = sc.gaussian_records(nrec % 2, nrec, 2, P, nvox)
        check_case(ctx, records, 1, range(P), f"P={P} nvox={nvox} nrec={nrec}")


@pytest.mark.parametrize("nrow, rows", [(2, [1, 0]), (3, [2, 0, 1]), (4, [2]), (4, [0, 3])])
def test_crlb_row_selection(ctx, nrow, rows):
    """permuted rows and strict subsets of the rows of a record"""
    for nrec, nvox in ((7, 65), (65, 63)):
        check_case(ctx, sc.gaussian_records(1, nrec, 2, nrow, nvox), 1, rows, f"rows={rows} nvox={nvox} nrec={nrec}")


def test_crlb_long_train(ctx):
    """1000 records over 65 voxels: eight wavefronts share the records of a voxel and meet in LDS; columns like a decaying
    signal and its derivatives, cond 1e4 .. 1e5"""
    records = sc.decaying_records(0)
    y = sc.Yardstick(sc.columns(records, 0, range(4)))
    assert y.keep.all() and y.cond.max() < 1e7, y.cond.max()
    check_case(ctx, records, 0, range(4), "nrec=1000")
    check_case(ctx, records, 0, [1], "nrec=1000 P=1")


@pytest.mark.parametrize("nrec", [7, 65, 1000])
def test_bits_do_not_depend_on_neighbours(ctx, nrec):
    """one voxel alone, the same voxel at position 200 of 257, and the same through the raw entry point with vox0 != 0"""
    from epgpy_amd import stats, _lib
    records = sc.gaussian_records(2, nrec, 2, 3, 257)
    whole = sc.upload_jacobian(ctx, records, 1, [2, 0, 1])
    alone = sc.upload_jacobian(ctx, np.ascontiguousarray(records[..., 200:201]), 1, [2, 0, 1])
    for kw in (dict(), dict(W=W4[:3], log=True)):
        a, b = stats.crlb(whole, **kw), stats.crlb(alone, **kw)
        assert a[200].tobytes() == b[0].tobytes(), (kw, a[200], b[0])
        a, b = stats.crlb_split(whole, **kw), stats.crlb_split(alone, **kw)
        assert a[:, 200].tobytes() == b[:, 0].tobytes(), kw
    part = _lib.signal_crlb(ctx, whole.ptr, whole.record_stride, whole.row_stride, 3, nrec, [2, 0, 1], 137, 100)
    assert part.shape == (100,) and part.tobytes() == stats.crlb(whole)[137:237].tobytes()
    part = _lib.signal_crlb(ctx, whole.ptr, whole.record_stride, whole.row_stride, 3, nrec, [2, 0, 1], 200, 1, split=True)
    assert part.tobytes() == stats.crlb_split(alone).tobytes()


def test_singular_voxel_is_nan(ctx):
    """an all-zero column in one voxel: NaN there, in crlb and in every row of crlb_split; the neighbours are untouched"""
    from epgpy_amd import stats
    records = sc.gaussian_records(3, 9, 2, 3, 130)
    clean = sc.upload_jacobian(ctx, records, 1, range(3))
    broken = records.copy()
    broken[:, 1, 1, 64] = 0.0
    jac = sc.upload_jacobian(ctx, broken, 1, range(3))
    others = np.arange(130) != 64
    for kw in (dict(), dict(log=True), dict(W=W4[:3])):
        got, ref = stats.crlb(jac, **kw), stats.crlb(clean, **kw)
        assert np.isnan(got[64]) and got[others].tobytes() == ref[others].tobytes(), kw
        got, ref = stats.crlb_split(jac, **kw), stats.crlb_split(clean, **kw)
        assert np.isnan(got[:, 64]).all() and got[:, others].tobytes() == ref[:, others].tobytes(), kw
    # P = 1: the zero column alone
    assert np.isnan(stats.crlb(sc.upload_jacobian(ctx, broken, 1, [1]))[64])


def test_end_to_end_mse(ctx):
    """12-echo multi-spin-echo train on a 5 x 7 (T2 x flip angle) grid: simulate(out="device") -> stats.crlb, against the
    yardstick on the downloaded Jacobian and against the host branch on it"""
    from epgpy_amd import epg, stats
    T2 = np.linspace(30.0, 120.0, 5)[:, None]
    alpha = np.linspace(110.0, 180.0, 7)[None, :]
    esp = 9.0
    necho = 12
    for variables, W in ((["magnitude", "T2"], [0.0, 1.0]), (["T2"], [1.0])):
        exc = epg.T(90, 90)
        rfc = epg.T(alpha, 0)
        rlx = epg.E(esp / 2, 1400.0, T2, order1=["T2"])
        seq = [exc] + [epg.S(1), rlx, rfc, epg.S(1), rlx, epg.ADC] * necho
        jac = epg.simulate(seq, probe=epg.Jacobian(variables), out="device")
        assert jac.shape == (necho, 5, 7, len(variables))
        host = np.asarray(jac)
        J = np.moveaxis(host, 0, -2)                               # [5, 7, necho, P]
        y = sc.Yardstick(J.reshape(35, necho, len(variables)))
        got = stats.crlb(jac, W=W)
        assert got.shape == (5, 7) and got.dtype == np.float64
        y.check(got.reshape(35), y.cost(W), what=f"mse {variables}")
        ref = stats.crlb(J, W=W)
        keep = y.keep.reshape(5, 7)
        assert np.all(np.abs(got - ref)[keep] <= (2 * y.tol.reshape(5, 7) * np.abs(ref))[keep])      # (each within tol of the yardstick)
        split = stats.crlb_split(jac, log=True)
        assert split.shape == (len(variables), 5, 7)
        y.check(split.reshape(len(variables), 35), y.split(), log=True, what=f"mse {variables} split log")


def test_released_handle_raises(ctx):
    from epgpy_amd import stats, _lib
    jac = sc.upload_jacobian(ctx, sc.gaussian_records(0, 5, 1, 2, 8), 0, range(2))
    jac._buf.free()
    with pytest.raises(_lib.EpgxError):
        stats.crlb(jac)
    with pytest.raises(_lib.EpgxError):
        np.asarray(jac)


def test_raw_entry_rejects_bad_arguments(ctx):
    """EPGX_ERR_INVALID (-1) and a message, nothing launched: `out` is still what it was"""
    from epgpy_amd import _lib
    records = sc.gaussian_records(0, 6, 1, 4, 32)
    jac = sc.upload_jacobian(ctx, records, 0, range(4))
    out = _lib.DeviceBuffer(ctx, 8 * 4 * 32, itemsize=8)
    marker = np.full(4 * 32, -7.0)
    out.upload(marker)

    def call(nparam=2, rows=(0, 1), nvox=32, vox0=0, nrow=4, nrec=6, sigma2=1.0, flags=0, w=None, record_stride=None):
        r = np.ascontiguousarray(list(rows) + [0] * 8, dtype=np.int32)
        wv = None if w is None else np.ascontiguousarray(w, dtype=np.float64)
        return ctx.lib.epgx_signal_crlb(ctx.handle, ctypes.c_void_p(jac.ptr), record_stride or jac.record_stride, jac.row_stride, nrow, nrec, nparam,
                                        r.ctypes.data, vox0, nvox, None if wv is None else wv.ctypes.data, sigma2, flags, out.ptr)

    for kw, word in ((dict(nparam=0), "nparam"), (dict(nparam=5, rows=(0, 1, 2, 3, 0)), "nparam"), (dict(rows=(0, 4)), "rows"),
                     (dict(nvox=-1), "voxels"), (dict(vox0=1), "voxels"), (dict(nrec=0), "nrec"), (dict(sigma2=0.0), "sigma2"),
                     (dict(flags=4), "flags"), (dict(nrow=5), "record_stride"), (dict(w=[1.0, np.inf]), "weights"),
                     (dict(record_stride=1 << 62), "overflow")):
        assert call(**kw) == -1, kw
        assert word in ctx.lib.epgx_last_error().decode(), (kw, ctx.lib.epgx_last_error())
    ctx.synchronize()
    assert np.array_equal(out.download(np.float64, (4 * 32,)), marker)
    assert call() == 0 and call(nvox=0) == 0
    got = out.download(np.float64, (32,))
    sc.Yardstick(sc.columns(records, 0, range(2))).check(got, sc.Yardstick(sc.columns(records, 0, range(2))).cost(), what="raw")

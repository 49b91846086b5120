"""GPU: stats.crlb_grad on a DeviceJacobian and a DeviceHessian (crlb_grad_kernel<P> through epgx_signal_crlb_grad) against the
reference's formula in extended precision (tests/stats_grad_cases.py: yardstick and the bar
max(64, nrec) * 2.2e-16 * cond2(I) * A_x per voxel and design variable; voxels with cond2 > 1e8 excluded, at most 10 %).

Shapes: the smallest at which the kernel can go wrong -- every P; nx = 1, one chunk (XB), one chunk and one (XB + 1, which
is 5 as well); voxel counts around one wavefront and one block (1, 63, 64, 65, 130), and a voxel range that starts inside a
longer row; record counts 1, CRLB_UNROLL -+ 1 and both sides of every threshold of crlb_slices (read from epgx_stats.h: one,
two, four, eight wavefronts per voxel, whose partial sums meet in LDS in rounds).  The Hessian's entries lie in passes of 3
and of 4 rows per record at two probe positions, some are absent (offset -1)."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import stats_cases as sc
from tests import stats_grad_cases as gc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_HEADER = open(os.path.join(ROOT, "epgpy_amd", "csrc", "epgx_stats.h")).read()


def _constant(name):
    return int(re.search(rf"constexpr int {name} = (\d+);", _HEADER).group(1))


XB, UNROLL, SLICE, MAX_SLICES = (_constant(n) for n in ("CRLB_GRAD_XB", "CRLB_UNROLL", "CRLB_SLICE", "CRLB_MAX_SLICES"))
NX = sorted({1, XB, XB + 1, 5})
NVOX = [1, 63, 64, 65, 130]
THRESHOLDS = [SLICE * s for s in (1, 2, 4, 8) if s < MAX_SLICES]          # crlb_slices doubles while slices * CRLB_SLICE < nrec
NREC = sorted({1, UNROLL - 1, UNROLL + 1} | {t + d for t in THRESHOLDS for d in (0, 1)})
SIGMA2 = 0.25


@pytest.fixture(scope="module")
def ctx():
    from epgpy_amd import _lib
    return _lib.get_context(0)


def missing_entries(P, nx):
    """a few absent entries: the magnitude row of every second design variable, and one more for P >= 3"""
    gone = {(0, x) for x in range(1, nx, 2)}
    if P >= 3 and nx >= 2:
        gone.add((2, 0))
    return gone


def make_case(seed, P, nrec, nvox, nx):
    """(J [nvox, nrec, P], H [nvox, nrec, P, nx] with zeros at the absent entries, the absent entries)"""
    J = sc.columns(sc.gaussian_records(seed, nrec, 2, P, nvox), 1, range(P))
    H = gc.gaussian_hessian(seed + 1, J, nx)
    gone = missing_entries(P, nx)
    for a, x in gone:
        H[:, :, a, x] = 0.0
    return J, H, gone


def upload_pair(ctx, J, H, gone):
    """the handles of J (probe 1 of 2 of its records) and H"""
    nvox, nrec, P = J.shape
    records = np.zeros((nrec, 2, P, nvox), dtype=np.complex128)
    records[:, 1] = np.moveaxis(J, (0, 1, 2), (2, 0, 1))
    records[:, 0] = 1e30
    return sc.upload_jacobian(ctx, records, 1, range(P)), gc.upload_hessian(ctx, H, gone)


def check_pair(ctx, J, H, gone, what):
    """plain and (W with a zero, sigma2 != 1, log) against the yardstick; the cost has the bits of stats.crlb.  Returns the
    handles and the two results.  Fewer records than parameters (nrec = 1 and CRLB_UNROLL - 1 at the larger P) leave an
    information matrix of rank nrec: every voxel is beyond the yardstick's cond2 limit, and neither NaN nor a value is
    specified there -- such a case still runs, and its cost must still have the bits of stats.crlb (NaN included)"""
    from epgpy_amd import stats
    nrec, P = J.shape[1:]
    jac, hes = upload_pair(ctx, J, H, gone)
    results = []
    for kw in (dict(), dict(W=gc.W4[:P], sigma2=SIGMA2, log=True)):
        cost, grad = stats.crlb_grad(jac, hes, **kw)
        assert cost.shape == J.shape[:1] and grad.shape == (J.shape[0], H.shape[-1]) and grad.dtype == np.float64
        if nrec >= P:
            y = gc.GradYardstick(J, H, W=kw.get("W"), sigma2=kw.get("sigma2", 1.0))
            y.check_cost(cost, log="log" in kw, what=what)
            y.check_grad(grad, log="log" in kw, what=what)
        assert cost.tobytes() == stats.crlb(jac, **kw).tobytes(), what
        results.append((cost, grad))
    return jac, hes, results


@pytest.mark.parametrize("nvox", NVOX)
@pytest.mark.parametrize("P", [1, 2, 3, 4])
def test_crlb_grad_gaussian(ctx, P, nvox):
    """every record count; nx cycles through NX with the record count, shifted by the voxel count, so that every nx meets
    every record count (at one voxel count or another)"""
    for i, nrec in enumerate(NREC):
        nx = NX[(i + NVOX.index(nvox)) % len(NX)]
        J, H, gone = make_case(nrec % 3, P, nrec, nvox, nx)
        check_pair(ctx, J, H, gone, f"P={P} nvox={nvox} nrec={nrec} nx={nx}")


@pytest.mark.parametrize("P", [1, 2, 3, 4])
def test_voxel_range_and_position_do_not_change_the_bits(ctx, P):
    """voxels [vox0, vox0 + nvox) inside a row of 130 through the raw entry; the same voxels uploaded alone (another
    position, another nvox): identical bits, within the bar"""
    from epgpy_amd import stats, _lib
    for nrec, nx in ((UNROLL + 1, XB + 1), (SLICE + 1, XB), (4 * SLICE + 1, 1)):
        J, H, gone = make_case(5, P, nrec, 130, nx)
        jac, hes, ((cost, grad), _) = check_pair(ctx, J, H, gone, f"P={P} nrec={nrec} nx={nx} whole row")
        for vox0, nvox in ((67, 63), (66, 64), (129, 1), (3, 65)):
            part_cost, part_grad = _lib.signal_crlb_grad(ctx, jac.ptr, jac.record_stride, jac.row_stride, jac._nrow, nrec, jac.rows, vox0, nvox,
                                                         hes.ptr, hes._buf.nbytes // 16, hes.offsets, hes.record_strides)
            assert part_cost.tobytes() == cost[vox0:vox0 + nvox].tobytes(), (nrec, vox0, nvox)
            assert part_grad.T.tobytes() == grad[vox0:vox0 + nvox].tobytes(), (nrec, vox0, nvox)
            if nvox < 64:
                a_jac, a_hes = upload_pair(ctx, J[vox0:vox0 + nvox], H[vox0:vox0 + nvox], gone)
                for kw in (dict(), dict(W=gc.W4[:P], sigma2=SIGMA2, log=True)):
                    a_cost, a_grad = stats.crlb_grad(a_jac, a_hes, **kw)
                    w_cost, w_grad = stats.crlb_grad(jac, hes, **kw)
                    assert a_cost.tobytes() == w_cost[vox0:vox0 + nvox].tobytes() and a_grad.tobytes() == w_grad[vox0:vox0 + nvox].tobytes()


@pytest.mark.parametrize("P", [2, 4])
def test_absent_entries_equal_explicit_zero_rows(ctx, P):
    from epgpy_amd import stats
    for nrec, nx in ((UNROLL + 1, XB + 1), (2 * SLICE + 1, XB)):
        J, H, gone = make_case(6, P, nrec, 65, nx)
        jac, hes = upload_pair(ctx, J, H, gone)
        _, full = upload_pair(ctx, J, H, ())
        assert (hes.offsets < 0).sum() == len(gone) > 0 and (full.offsets >= 0).all()
        for kw in (dict(), dict(W=gc.W4[:P], sigma2=SIGMA2, log=True)):
            a, b = stats.crlb_grad(jac, hes, **kw), stats.crlb_grad(jac, full, **kw)
            assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


@pytest.mark.parametrize("P", [2, 3, 4])
def test_equal_columns_give_nan(ctx, P):
    """voxel 64 of 130 gets two equal Jacobian columns: NaN in its cost and in all nx gradient entries, the neighbours keep
    their bits.  The columns are chosen so that the zero pivot is exact (one entry 2 in record 0, where the other columns are
    0: the Gram entries are 4 and 0, the factor's 2 and 0); equal columns in general position leave a pivot of a few ulp of
    either sign, where neither the reference nor the kernel promises NaN (epgpy_amd/stats.py, module docstring)."""
    from epgpy_amd import stats
    nrec, nx = SLICE + 1, XB + 1
    J, H, gone = make_case(8, P, nrec, 130, nx)
    _, _, ((cost, grad), (lcost, lgrad)) = check_pair(ctx, J, H, gone, f"P={P} clean")
    broken = J.copy()
    broken[64, 0, :] = 0.0
    broken[64, :, P - 2:] = 0.0
    broken[64, 0, P - 2:] = 2.0
    jac, hes = upload_pair(ctx, broken, H, gone)
    others = np.arange(130) != 64
    for kw, (c0, g0) in ((dict(), (cost, grad)), (dict(W=gc.W4[:P], sigma2=SIGMA2, log=True), (lcost, lgrad))):
        c, g = stats.crlb_grad(jac, hes, **kw)
        assert np.isnan(c[64]) and np.isnan(g[64]).all() and g[64].shape == (nx,), kw
        assert c[others].tobytes() == c0[others].tobytes() and g[others].tobytes() == g0[others].tobytes(), kw
        assert np.isnan(stats.crlb(jac, **kw)[64])


def test_entry_refuses_an_entry_that_ends_past_the_buffer(ctx):
    """hess_len one element short of the last record of the last entry: EPGX_ERR_INVALID, nothing launched (the outputs keep
    their marker); the exact length passes"""
    from epgpy_amd import _lib
    nrec, nvox, P, nx = 6, 32, 2, 3
    J, H, gone = make_case(9, P, nrec, nvox, nx)
    jac, hes = upload_pair(ctx, J, H, gone)
    live = hes.offsets >= 0
    need = int((hes.offsets + (nrec - 1) * hes.record_strides)[live].max()) + nvox
    assert need <= hes._buf.nbytes // 16
    with pytest.raises(_lib.EpgxError, match="epgx_signal_crlb_grad"):
        _lib.signal_crlb_grad(ctx, jac.ptr, jac.record_stride, jac.row_stride, jac._nrow, nrec, jac.rows, 0, nvox, hes.ptr, need - 1,
                              hes.offsets, hes.record_strides)
    out = _lib.DeviceBuffer(ctx, 8 * (1 + nx) * nvox, itemsize=8)
    marker = np.full((1 + nx) * nvox, -7.0)
    out.upload(marker)
    rows = np.ascontiguousarray(jac.rows, dtype=np.int32)
    off, step = np.ascontiguousarray(hes.offsets, dtype=np.int64), np.ascontiguousarray(hes.record_strides, dtype=np.int64)

    def call(hess_len=need, vox0=0, nvox_=nvox, flags=0, nx_=nx, steps=step):
        return ctx.lib.epgx_signal_crlb_grad(ctx.handle, ctypes.c_void_p(jac.ptr), jac.record_stride, jac.row_stride, jac._nrow, nrec, P,
                                             rows.ctypes.data, vox0, nvox_, ctypes.c_void_p(hes.ptr), hess_len, nx_, off.ctypes.data,
                                             steps.ctypes.data, None, 1.0, flags, out.ptr, ctypes.c_void_p(out.ptr.value + 8 * nvox))

    short = np.where(live, nvox - 1, 0).astype(np.int64)
    for kw, word in ((dict(hess_len=need - 1), "hess_len"), (dict(vox0=1, nvox_=nvox - 1, hess_len=need - 1), "hess_len"),
                     (dict(steps=short), "overlap"), (dict(flags=1), "flags"), (dict(nx_=0), "nx"), (dict(hess_len=-1), "hess_len")):
        assert call(**kw) == -1, kw
        assert word in ctx.lib.epgx_last_error().decode(), (kw, ctx.lib.epgx_last_error())
    ctx.synchronize()
    assert np.array_equal(out.download(np.float64, ((1 + nx) * nvox,)), marker)
    assert call() == 0 and call(nvox_=0) == 0
    got = out.download(np.float64, (1 + nx, nvox))
    y = gc.GradYardstick(J, H)
    y.check_cost(got[0], what="raw")
    y.check_grad(np.ascontiguousarray(got[1:].T), what="raw")


def test_end_to_end_echo_train(ctx):
    """the 6-echo train of tests/test_gpu_hessian_device.py over 5 T2 values: Jacobian and Hessian handles from two calls ->
    stats.crlb_grad, against the yardstick fed with the downloaded handles"""
    from epgpy_amd import epg, stats, functions
    rf = epg.T(150.0, 0.0, order1={"fa": {"alpha": 1.0}}, order2=[("fa", "fa"), ("T2", "fa")])
    rl = epg.E(5.0, 1000.0, np.linspace(40.0, 90.0, 5), order1="T2", order2=[("T2", "T2"), ("T2", "fa")])
    seq = [epg.T(90.0, 90.0)] + [epg.S(1), rl, rf, epg.S(1), rl, epg.ADC] * 6
    J_dev = epg.simulate(seq, probe=epg.Jacobian(["magnitude", "T2"]), out="device")
    H_dev = epg.simulate(seq, probe=epg.Hessian(["magnitude", "T2"], ["fa"]), mode="resident", out="device")
    assert isinstance(J_dev, functions.DeviceJacobian) and isinstance(H_dev, functions.DeviceHessian)
    J = np.moveaxis(np.asarray(J_dev), 0, -2)                    # [5, 6, 2]
    H = np.moveaxis(np.asarray(H_dev), 0, -3)                    # [5, 6, 2, 1]
    assert J.shape == (5, 6, 2) and H.shape == (5, 6, 2, 1) and np.abs(H).max() > 0
    for kw in (dict(W=[0.0, 1.0], sigma2=1e-4, log=True), dict()):
        y = gc.GradYardstick(J, H, W=kw.get("W"), sigma2=kw.get("sigma2", 1.0))
        cost, grad = stats.crlb_grad(J_dev, H_dev, **kw)
        assert cost.shape == (5,) and grad.shape == (5, 1)
        y.check_cost(cost, log="log" in kw, what="echo train")
        y.check_grad(grad, log="log" in kw, what="echo train")
        assert cost.tobytes() == stats.crlb(J_dev, **kw).tobytes()
    with pytest.raises(NotImplementedError, match="crlb_grad"):
        stats.crlb(J_dev, H=H_dev)

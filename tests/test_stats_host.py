"""CPU: epgpy_amd.stats on host arrays against the reference's outputs (tests/golden/g21_stats.npz, written by
tests/golden/make_golden_stats.py), the Student t quantile, the C boundary of epgx_signal_crlb and the argument checks of the
device branch that need no GPU.

Tolerance of the golden comparison: 1e-12 relative.  The host functions evaluate the reference's formulas with the same LAPACK
underneath; what differs is the order of a few roundings."""
import os
import re

import numpy as np
import pytest

from epgpy_amd import stats, functions, _lib, _build
from tests import stats_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL = 1e-12


@pytest.fixture(scope="module")
def g21():
    return np.load(os.path.join(ROOT, "tests", "golden", "g21_stats.npz"))


def close(got, ref):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape and got.dtype == ref.dtype, (got.shape, ref.shape, got.dtype, ref.dtype)
    assert np.all(np.abs(got - ref) <= RTOL * np.abs(ref)), float(np.max(np.abs(got - ref) / np.abs(ref)))


def test_crlb_golden(g21):
    J, W = g21["crlb_J"], g21["crlb_W"]
    close(stats.crlb(J), g21["crlb_plain"])
    close(stats.crlb(J, W=W, sigma2=0.3, log=True), g21["crlb_w_log"])
    close(stats.crlb(J, W=g21["crlb_Wmap"]), g21["crlb_wmap"])


def test_crlb_gradient_golden(g21):
    J, H = g21["grad_J"], g21["grad_H"]
    cost, grad = stats.crlb(J, H)
    close(cost, g21["grad_cost"])
    close(grad, g21["grad_grad"])
    cost, grad = stats.crlb(J, H, W=g21["grad_W"], sigma2=1.7, log=True)
    close(cost, g21["grad_cost_w_log"])
    close(grad, g21["grad_grad_w_log"])


def test_crlb_split_golden(g21):
    J, W = g21["crlb_J"], g21["crlb_W"]
    close(stats.crlb_split(J), g21["split_plain"])
    close(stats.crlb_split(J, W=W[[0, 1, 2, 4, 4]], sigma2=0.3, log=True), g21["split_w_log"])
    assert stats.crlb_split(J).shape == (5, 3, 2)


def test_confint_golden(g21):
    obs, pred, jac, hess = g21["ci_obs"], g21["ci_pred"], g21["ci_jac"], g21["ci_hess"]
    for level, tag in ((0.99, "99"), (0.8, "8")):
        cints, cband = stats.confint(obs, pred, jac, conflevel=level)
        close(cints, g21[f"ci_cints_{tag}"])
        close(cband, g21[f"ci_cband_{tag}"])
        cints, cband = stats.confint(obs, pred, jac, hess, conflevel=level)
        close(cints, g21[f"ci_cints_hess_{tag}"])
        close(cband, g21[f"ci_cband_hess_{tag}"])


def test_host_branch_meets_the_device_tolerance():
    """the float64 formula against the extended-precision yardstick of the GPU tests, at their tolerance: what the device is
    held to is what the reference's own arithmetic achieves"""
    for seed, nrec, P in ((0, 7, 4), (1, 64, 3), (0, 5, 1)):
        J = sc.columns(sc.gaussian_records(seed, nrec, 1, P, 65), 0, range(P))
        y = sc.Yardstick(J)
        y.check(stats.crlb(J), y.cost(), what="host crlb")
        y.check(stats.crlb_split(J, log=True), y.split(), log=True, what="host split log")
    records = sc.decaying_records(0)
    y = sc.Yardstick(sc.columns(records, 0, range(4)))
    assert y.keep.all() and 1e3 < y.cond.max() < 1e7
    y.check(stats.crlb(sc.columns(records, 0, range(4))), y.cost(), what="host decaying")


def test_gauss_jordan_inverse():
    rng = np.random.default_rng(5)
    A = rng.standard_normal((9, 4, 4))
    A[0, 0, 0] = 0.0                              # needs the pivot search
    assert np.allclose(sc.gauss_jordan_inverse(A).astype(np.float64), np.linalg.inv(A), rtol=1e-10, atol=1e-12)


def test_zero_column_gives_nan():
    rng = np.random.default_rng(3)
    J = rng.standard_normal((4, 8, 3)) + 1j * rng.standard_normal((4, 8, 3))
    J[2, :, 1] = 0.0
    with np.errstate(all="ignore"):
        cost, split = stats.crlb(J), stats.crlb_split(J)
    assert np.isnan(cost[2]) and np.isnan(split[:, 2]).all()
    others = [0, 1, 3]
    assert np.isfinite(cost[others]).all() and np.isfinite(split[:, others]).all()


def test_t_interval_against_scipy():
    scipy_stats = pytest.importorskip("scipy.stats")
    for level in (0.95, 0.99):
        for dof in range(1, 201):
            ref = scipy_stats.t.interval(level, dof)[1]
            assert abs(stats._t_interval(level, dof) - ref) <= 1e-10 * ref, (level, dof)


def test_t_interval_against_mpmath():
    """the quantile against a 40-digit root of the same tail probability: 1e-13 relative"""
    mp = pytest.importorskip("mpmath")
    with mp.workdps(40):
        for level, dof in ((0.95, 1), (0.95, 9), (0.99, 9), (0.99, 10), (0.8, 10), (0.95, 57), (0.99, 200), (0.5, 3)):
            tail = 1 - mp.mpf(repr(level))
            ref = mp.findroot(lambda t: mp.betainc(mp.mpf(dof) / 2, mp.mpf(1) / 2, 0, dof / (dof + t * t), regularized=True) - tail,
                              mp.mpf(stats._t_interval(level, dof)))
            assert abs(stats._t_interval(level, dof) - ref) <= 1e-13 * ref, (level, dof)


def test_t_interval_known_values():
    """textbook values (two-sided 95 % / 99 %)"""
    assert abs(stats._t_interval(0.95, 1) - 12.706204736) < 1e-8       # tan(0.475 pi)
    assert abs(stats._t_interval(0.95, 1) - np.tan(0.475 * np.pi)) < 1e-11
    assert abs(stats._t_interval(0.99, 2) - 9.924843201) < 1e-8        # dof 2 in closed form: p sqrt(2 / (1 - p^2))
    assert abs(stats._t_interval(0.99, 2) - 0.99 * np.sqrt(2 / (1 - 0.99 ** 2))) < 1e-11
    assert abs(stats._t_interval(0.95, 1e7) - 1.959963985) < 1e-6      # the normal limit
    with pytest.raises(ValueError):
        stats._t_interval(1.0, 3)
    with pytest.raises(ValueError):
        stats._t_interval(0.95, 0)


def test_boundary_agrees():
    """include/epgx.h, _lib.py and the built library: epgx_signal_crlb and ABI 11"""
    header = open(os.path.join(ROOT, "include", "epgx.h")).read()
    assert "#define EPGX_ABI_VERSION 11" in header and _lib.ABI_VERSION == 11
    proto = re.search(r"int epgx_signal_crlb\(([^)]*)\)", header).group(1)
    assert len(proto.split(",")) == len(_lib.SYMBOLS["epgx_signal_crlb"][1]) == 14
    assert re.search(rf"EPGX_CRLB_SPLIT = {_lib.CRLB_SPLIT}, EPGX_CRLB_LOG10 = {_lib.CRLB_LOG10}", header)
    lib = _lib.load()
    assert lib.epgx_abi_version() == 11 and hasattr(lib, "epgx_signal_crlb")
    assert any(src == "epgx_stats.hip" for _, src, _ in _build.UNITS)
    assert "epgx_signal_crlb" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_raw_entry_validates_before_any_device_work():
    """NULL arguments are refused without a context: EPGX_ERR_INVALID and a message"""
    lib = _lib.load()
    assert lib.epgx_signal_crlb(None, None, 0, 0, 1, 1, 1, None, 0, 0, None, 1.0, 0, None) == -1
    assert b"epgx_signal_crlb" in lib.epgx_last_error()


class _Ptr:
    value = 1 << 20


class _Buf:
    """stands in for a DeviceBuffer: the checks under test raise before anything touches it"""
    class ctx:
        device = 0
    ptr = _Ptr()


def test_device_branch_argument_errors():
    jac = functions.DeviceJacobian(_Buf(), 6, (5, 7), 1, 3, 0, [0, 2], ["magnitude", "T2"])
    H = np.zeros((5, 7, 6, 2, 1))
    with pytest.raises(NotImplementedError, match="H"):
        stats.crlb(jac, H)
    with pytest.raises(NotImplementedError, match="W"):
        stats.crlb(jac, W=np.ones((5, 7, 2)))
    with pytest.raises(NotImplementedError, match="W"):
        stats.crlb_split(jac, W=np.ones((7, 2)))
    with pytest.raises(NotImplementedError, match="W"):
        stats.crlb(jac, W=np.ones(3))
    with pytest.raises(NotImplementedError, match="sigma2"):
        stats.crlb(jac, sigma2=np.ones((5, 7)))
    with pytest.raises(NotImplementedError, match="sigma2"):
        stats.crlb_split(jac, sigma2=np.ones((5, 7, 1, 1)))
    part = functions.DeviceSignal(_Buf(), 6, (5, 7), 0, 1, vox0=0, count=20)
    sharded = functions.ShardedDeviceSignal([part], (5, 7))
    for fn in (stats.crlb, stats.crlb_split):
        with pytest.raises(NotImplementedError, match="J"):
            fn(sharded)
        with pytest.raises(NotImplementedError, match="J"):
            fn(part)
    with pytest.raises(NotImplementedError):
        stats.confint(jac, jac, jac)

"""CPU: stats.crlb_grad -- the C boundary of epgx_signal_crlb_grad, the argument checks of the device branch on stub handles
(raised before anything touches a buffer), the host-array case (exactly stats.crlb(J, H=H)), the float64 formula against the
extended-precision yardstick of the GPU tests at their bar (tests/stats_grad_cases.py), and the reference's own gradient
(the H case of tests/golden/g21_stats.npz)."""
import os
import re

import numpy as np
import pytest

from epgpy_amd import stats, functions, _lib
from tests import stats_cases as sc
from tests import stats_grad_cases as gc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_boundary_agrees():
    """include/epgx.h, _lib.py, the built library and INTEGRATION.md: epgx_signal_crlb_grad inside ABI 11"""
    header = open(os.path.join(ROOT, "include", "epgx.h")).read()
    assert "#define EPGX_ABI_VERSION 11" in header and _lib.ABI_VERSION == 11
    proto = re.search(r"int epgx_signal_crlb_grad\(([^)]*)\)", header).group(1)
    assert len(proto.split(",")) == len(_lib.SYMBOLS["epgx_signal_crlb_grad"][1]) == 20
    lib = _lib.load()
    assert lib.epgx_abi_version() == 11 and hasattr(lib, "epgx_signal_crlb_grad")
    assert "epgx_signal_crlb_grad" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    stats_h = open(os.path.join(ROOT, "epgpy_amd", "csrc", "epgx_signal_limits.h")).read()
    assert re.search(rf"CRLB_MAX_P = {stats.MAX_DEVICE_PARAMS};", stats_h)


def test_raw_entry_validates_before_any_device_work():
    """NULL arguments are refused without a context: EPGX_ERR_INVALID and a message that names the entry"""
    lib = _lib.load()
    assert lib.epgx_signal_crlb_grad(None, None, 0, 0, 1, 1, 1, None, 0, 0, None, 0, 1, None, None, None, 1.0, 0, None, None) == -1
    assert b"epgx_signal_crlb_grad" in lib.epgx_last_error()


def stub_pair(grid=(5, 7), nrec=6, variables=("magnitude", "T2"), nx=3, buf_j=None, buf_h=None, hgrid=None, hnrec=None, hvariables=None):
    buf_j = buf_j or gc.StubBuffer()
    P = len(variables)
    jac = functions.DeviceJacobian(buf_j, nrec, grid, 1, P + 1, 0, list(range(P)), list(variables))
    hgrid = hgrid or grid
    hes, _ = gc.hessian_handle(buf_h or buf_j, (int(np.prod(hgrid)), hnrec or nrec, len(hvariables or variables), nx), grid=hgrid,
                               variables1=list(hvariables or variables))
    return jac, hes


def test_device_branch_argument_errors():
    jac, hes = stub_pair()
    other = gc.StubBuffer()
    with pytest.raises(ValueError, match="H"):                                 # another context
        stats.crlb_grad(*stub_pair(buf_h=other))
    with pytest.raises(ValueError, match="H"):                                 # another device
        stats.crlb_grad(*stub_pair(buf_h=gc.StubBuffer(device=1)))
    with pytest.raises(ValueError, match="H"):
        stats.crlb_grad(*stub_pair(hgrid=(7, 5)))
    with pytest.raises(ValueError, match="H"):
        stats.crlb_grad(*stub_pair(hnrec=5))
    with pytest.raises(ValueError, match="variables1"):
        stats.crlb_grad(*stub_pair(hvariables=("T2", "magnitude")))
    with pytest.raises(ValueError, match="variables1"):
        stats.crlb_grad(*stub_pair(hvariables=("magnitude",)))
    with pytest.raises(NotImplementedError, match="W"):
        stats.crlb_grad(jac, hes, W=np.ones((5, 7, 2)))
    with pytest.raises(NotImplementedError, match="W"):
        stats.crlb_grad(jac, hes, W=np.ones(3))
    with pytest.raises(NotImplementedError, match="sigma2"):
        stats.crlb_grad(jac, hes, sigma2=np.ones((5, 7)))
    with pytest.raises(NotImplementedError, match="J"):                        # five parameters
        stats.crlb_grad(*stub_pair(variables=("magnitude", "T2", "T1", "B1", "g")))
    part = functions.DeviceSignal(gc.StubBuffer(), 6, (5, 7), 0, 1, vox0=0, count=20)
    sharded = functions.ShardedDeviceSignal([part], (5, 7))
    for bad in (part, sharded, hes):
        with pytest.raises(NotImplementedError, match="J"):
            stats.crlb_grad(bad, hes)
    for bad in (part, sharded, jac):
        with pytest.raises(NotImplementedError, match="H"):
            stats.crlb_grad(jac, bad)
    # one handle, one array: says which to download
    with pytest.raises(NotImplementedError, match="download J"):
        stats.crlb_grad(jac, np.zeros((5, 7, 6, 2, 3)))
    with pytest.raises(NotImplementedError, match="download H"):
        stats.crlb_grad(np.zeros((5, 7, 6, 2)), hes)


def test_crlb_on_handles_points_to_crlb_grad():
    jac, hes = stub_pair()
    with pytest.raises(NotImplementedError, match="H.*crlb_grad"):
        stats.crlb(jac, H=hes)


def test_array_inputs_equal_crlb():
    J = sc.columns(sc.gaussian_records(4, 9, 1, 3, 11), 0, range(3))
    H = gc.gaussian_hessian(5, J, 4)
    for kw in (dict(), dict(W=gc.W4[:3], sigma2=0.3, log=True), dict(W=np.ones((11, 3)), sigma2=np.full((11, 1, 1), 2.0))):
        cost, grad = stats.crlb_grad(J, H, **kw)
        ref_cost, ref_grad = stats.crlb(J, H=H, **kw)
        assert cost.tobytes() == ref_cost.tobytes() and grad.tobytes() == ref_grad.tobytes() and grad.shape == (11, 4)


def host_cases():
    for seed, nrec, nrow, nvox in ((0, 21, 5, 200), (1, 67, 3, 130)):
        yield f"gaussian nrec={nrec} P={nrow}", sc.columns(sc.gaussian_records(seed, nrec, 1, nrow, nvox), 0, range(nrow))
    yield "decaying", sc.columns(sc.decaying_records(3), 0, range(4))


def test_host_branch_meets_the_device_bar():
    """the float64 formula against the extended-precision yardstick, at the bar the device is held to"""
    for what, J in host_cases():
        P = J.shape[-1]
        H = gc.gaussian_hessian(7, J, 5)
        W = np.concatenate([gc.W4, [0.7]])[:P]
        for kw in (dict(), dict(W=W, sigma2=0.25, log=True)):
            y = gc.GradYardstick(J, H, W=kw.get("W"), sigma2=kw.get("sigma2", 1.0))
            assert y.keep.all(), what
            cost, grad = stats.crlb_grad(J, H, **kw)
            y.check_cost(cost, log="log" in kw, what=f"host {what}")
            y.check_grad(grad, log="log" in kw, what=f"host {what}")


def test_yardstick_against_finite_differences():
    """the yardstick's gradient is the derivative of the yardstick's cost: central differences along H, 1e-6 relative to the
    magnitude sum A_x"""
    J = sc.columns(sc.gaussian_records(2, 12, 1, 3, 6), 0, range(3))
    H = gc.gaussian_hessian(3, J, 2)
    y = gc.GradYardstick(J, H, W=gc.W4[:3], sigma2=0.5)
    step = 1e-5
    for x in range(2):
        up = sc.Yardstick(J + step * H[..., x], sigma2=0.5).cost(gc.W4[:3])
        dn = sc.Yardstick(J - step * H[..., x], sigma2=0.5).cost(gc.W4[:3])
        fd = (up - dn) / (2 * step)
        scale = y.bar[:, x] / (max(64, 12) * sc.EPS * y.cond)          # A_x
        assert np.all(np.abs(fd - y.grad[:, x]) <= 1e-6 * scale), float(np.max(np.abs(fd - y.grad[:, x]) / scale))


def test_reference_gradient_golden():
    """the gradient the reference computed (H case of golden G21): 1e-12 relative, as tests/test_stats_host.py holds crlb to"""
    g21 = np.load(os.path.join(ROOT, "tests", "golden", "g21_stats.npz"))
    J, H = g21["grad_J"], g21["grad_H"]
    for kw, tag in ((dict(), ""), (dict(W=g21["grad_W"], sigma2=1.7, log=True), "_w_log")):
        cost, grad = stats.crlb_grad(J, H, **kw)
        for got, ref in ((cost, g21["grad_cost" + tag]), (grad, g21["grad_grad" + tag])):
            assert got.shape == ref.shape and np.all(np.abs(got - ref) <= 1e-12 * np.abs(ref))

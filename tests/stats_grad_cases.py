"""Helpers of tests/test_stats_grad_host.py and tests/test_gpu_stats_grad.py: the gradient form of the Cramer-Rao bound in
extended precision (the yardstick), the tolerance derived from it, and synthetic second derivatives laid out as the passes of a
Hessian call leave them in HBM.  Builds on tests/stats_cases.py (Gauss-Jordan inverse, `cond`, `keep`, `tol` of the cost).

Yardstick.  The reference's formula (epgpy/stats.py:31-33) on `clongdouble`:
    I = Re(J^H J) / sigma2,  lb = I^-1,  S = lb diag(W) lb,
    G_x[a][b] = sum_k Re( conj(H_kax) J_kb ),   grad_x = -(2 / sigma2) sum_ab S_ab G_x[a][b].

Tolerance, per voxel and design variable, absolute:
    bar = max(64, nrec) * 2.2e-16 * cond2(I) * A_x,     A_x = (2 / sigma2) * max|S| * sum_k sum_ab |H_kax| |J_kb|.
A_x is the gradient's sum with every term replaced by its magnitude; the sequential sums err by nrec * eps of that magnitude
and S by a small multiple of P * eps * cond (the Cholesky inverse).  With `log` the result is `grad / (cost ln 10)`: it is
multiplied by the YARDSTICK's cost and ln 10 and compared in the same way.  Voxels with cond2(I) > 1e8 are excluded; at most
10 % of a case may be.
"""
import numpy as np

from tests import stats_cases as sc

W4 = np.array([0.5, 0.0, 1.25, 3.0])      # a zero and unequal weights (P = 1: 0.5 alone, the cost must stay positive for log)


class GradYardstick(sc.Yardstick):
    """J [nvox, nrec, P], H [nvox, nrec, P, nx] complex128 -> the cost's yardstick (sc.Yardstick) plus .grad [nvox, nx]
    (longdouble, never logged) and .bar [nvox, nx]"""

    def __init__(self, J, H, W=None, sigma2=1.0):
        super().__init__(J, sigma2=sigma2)
        J, H = np.asarray(J), np.asarray(H)
        assert H.shape[:3] == J.shape and H.ndim == 4, (J.shape, H.shape)
        self.W = np.ones(J.shape[-1]) if W is None else np.asarray(W, dtype=np.float64)
        Jl, Hl = J.astype(np.clongdouble), H.astype(np.clongdouble)
        s2 = np.longdouble(sigma2)
        info = np.einsum("vnp,vnq->vpq", Jl.conj(), Jl).real / s2
        with np.errstate(all="ignore"):
            lb = sc.gauss_jordan_inverse(info)
            S = np.einsum("vap,p,vpb->vab", lb, self.W.astype(np.longdouble), lb)
            G = np.einsum("vkax,vkb->vxab", Hl.conj(), Jl).real
            self.grad = -(2 / s2) * np.einsum("vab,vxab->vx", S, G)
            mag = np.einsum("vkax,vkb->vx", np.abs(H), np.abs(J))
            A = 2.0 / float(sigma2) * np.abs(S).max(axis=(-2, -1)).astype(np.float64)[:, None] * mag
            self.bar = max(64, J.shape[1]) * sc.EPS * self.cond[:, None] * A

    def check_cost(self, got, log=False, what=""):
        self.check(got, self.cost(self.W), log=log, what=f"{what} cost")

    def check_grad(self, got, log=False, what=""):
        """got [nvox, nx] float64 (the gradient of log10(cost) if `log`)"""
        got = np.asarray(got)
        assert got.dtype == np.float64 and got.shape == self.grad.shape, (what, got.dtype, got.shape, self.grad.shape)
        excluded = 1.0 - self.keep.mean()
        assert excluded <= sc.EXCLUDED_MAX, f"{what}: {excluded:.0%} of the voxels have cond > {sc.COND_MAX:g}"
        assert np.all(np.isfinite(got[self.keep])), what
        val = got.astype(np.longdouble)
        if log:
            val = val * self.cost(self.W)[:, None] * np.log(np.longdouble(10))
        err = np.abs(val - self.grad).astype(np.float64)
        with np.errstate(all="ignore"):      # (a bar of 0 -- every H entry of the variable absent or zero -- admits the exact 0 alone)
            ratio = np.where(self.keep[:, None] & (err > 0), err / self.bar, 0.0)
        worst = float(np.max(ratio))
        print(f"{what} grad{' log' if log else ''}: max err / bar = {worst:.3g} (cond up to {float(self.cond[self.keep].max()):.3g}, "
              f"{excluded:.0%} excluded)")
        assert worst <= 1.0, (what, worst)


def gaussian_hessian(seed, J, nx):
    """H [nvox, nrec, P, nx]: standard-normal complex entries scaled to |J| of their record and column"""
    rng = np.random.default_rng(seed)
    shape = J.shape + (nx,)
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) * np.abs(J)[..., None]


class StubBuffer:
    """stands in for a DeviceBuffer where the checks under test raise before anything touches it"""

    class _Ptr:
        value = 1 << 20

    def __init__(self, device=0, nbytes=1 << 30):
        self.ctx = type("ctx", (), {"device": device})()
        self.ptr = self._Ptr()
        self.nbytes = nbytes


def hessian_handle(buf, H_shape, missing=(), grid=None, variables1=None, variables2=None):
    """(DeviceHessian on `buf`, the entries it stores) for second derivatives H [nvox, nrec, P, nx] in a stub layout: passes
    of 3 and of 4 rows per record alternate, two probe positions per record; the entries (a, x) that are not in `missing`
    fill, one after the other, the last row of position 0 and of position 1 of a pass; those in `missing` are at offset -1"""
    from epgpy_amd import functions
    nvox, nrec, P, nx = H_shape
    entries = [(a, x) for a in range(P) for x in range(nx) if (a, x) not in set(missing)]
    passes = [(f"u{i}", f"u{i}") if i % 2 == 0 else (f"u{i}", f"w{i}") for i in range((len(entries) + 1) // 2)]
    nprobe, stride = 2, nrec * 2 * 4
    layout = functions._HessianLayout(passes, stride, nprobe, (nvox,) if grid is None else tuple(grid), nrec)
    where = np.full((P, nx, 2), -1, dtype=np.int64)
    for i, (a, x) in enumerate(entries):
        where[a, x] = (i // 2, layout.row(i // 2, 0, i % 2, layout.nrow(i // 2) - 1))
    handle = functions.DeviceHessian(buf, layout, where, variables1 or [f"v{a}" for a in range(P)], variables2 or [f"x{x}" for x in range(nx)])
    return handle, entries


def upload_hessian(ctx, H, missing=(), grid=None, variables1=None):
    """H [nvox, nrec, P, nx] in a DeviceBuffer [pass][row][voxel], wrapped as a DeviceHessian (hessian_handle); the rows that
    belong to no entry hold 1e30 (1 + i), so that a wrong address shows.  The entries in `missing` are not stored: H must be
    zero there"""
    from epgpy_amd import _lib
    H = np.asarray(H)
    nvox, nrec, P, nx = H.shape
    npass = (P * nx - len(set(missing)) + 1) // 2
    buf = _lib.DeviceBuffer(ctx, max(npass, 1) * nrec * 2 * 4 * nvox * 16)
    handle, entries = hessian_handle(buf, H.shape, missing, grid, variables1)
    flat = np.full(buf.nbytes // 16, 1e30 * (1 + 1j), dtype=np.complex128)
    for a, x in entries:
        off, step = int(handle.offsets[a, x]), int(handle.record_strides[a, x])
        for n in range(nrec):
            flat[off + n * step: off + n * step + nvox] = H[:, n, a, x]
    for a, x in set(missing):
        assert not H[:, :, a, x].any()
    buf.upload(flat)
    return handle

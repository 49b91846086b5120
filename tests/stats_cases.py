"""Helpers of tests/test_gpu_stats.py: the Cramer-Rao formula in extended precision (the yardstick), the tolerance derived
from it, and synthetic Jacobians laid out as a Jacobian probe leaves them in HBM.

Yardstick.  `I = 1 / sigma2 Re(J^H J)` with `einsum` on `clongdouble`, its inverse with a hand-written Gauss-Jordan elimination
(`np.linalg` has no long double; P <= 4), cost and per-column bounds from that -- the reference's formula (epgpy/stats.py:6-54)
at 64-bit mantissa.

Tolerance, per voxel and relative to the yardstick: `max(64, nrec) * 2.2e-16 * cond2(I)`.  A sequential fp64 sum of nrec terms
errs by at most nrec * eps relative to the sum of magnitudes (here all diagonal terms are positive, and the off-diagonal ones
are bounded by the diagonal), a Cholesky inverse by a small multiple of P * eps * cond.  For a log10 result `y = log10(x)` the
same relative bound `t` on x is an absolute bound `t / ln 10` on y.
Voxels with cond2(I) > 1e8 are excluded; at most 10 % of a case may be.
"""
import numpy as np

EPS = 2.2e-16
COND_MAX = 1e8
EXCLUDED_MAX = 0.10


def gauss_jordan_inverse(A):
    """inverse of every matrix of A [..., P, P] (np.longdouble), Gauss-Jordan with partial pivoting"""
    A = np.array(A, dtype=np.longdouble)
    lead, P = A.shape[:-2], A.shape[-1]
    A = A.reshape((-1, P, P))
    n = A.shape[0]
    aug = np.concatenate([A, np.broadcast_to(np.eye(P, dtype=np.longdouble), A.shape)], axis=-1)
    idx = np.arange(n)
    for col in range(P):
        piv = col + np.argmax(np.abs(aug[:, col:, col]), axis=1)
        swap = aug[idx, piv].copy()
        aug[idx, piv] = aug[:, col]
        aug[:, col] = swap
        aug[:, col] = aug[:, col] / aug[:, col, col][:, None]
        for row in range(P):
            if row != col:
                aug[:, row] = aug[:, row] - aug[:, row, col][:, None] * aug[:, col]
    return aug[:, :, P:].reshape(lead + (P, P))


class Yardstick:
    """J [nvox, nrec, P] complex128 -> .lb [nvox, P] (diagonal of the inverse information matrix, longdouble), .cond [nvox]
    (2-norm condition of the float64 information matrix), .keep (voxels inside COND_MAX), .tol [nvox]"""

    def __init__(self, J, sigma2=1.0):
        J = np.asarray(J)
        Jl = J.astype(np.clongdouble)
        info = np.einsum("vnp,vnq->vpq", Jl.conj(), Jl).real / np.longdouble(sigma2)
        with np.errstate(all="ignore"):
            self.lb = np.diagonal(gauss_jordan_inverse(info), axis1=-2, axis2=-1)
            self.cond = np.linalg.cond(info.astype(np.float64))
        self.keep = self.cond <= COND_MAX
        self.tol = max(64, J.shape[1]) * EPS * self.cond

    def cost(self, W=None):
        w = np.ones(self.lb.shape[-1]) if W is None else np.asarray(W)
        return (self.lb * w.astype(np.longdouble)).sum(-1)

    def split(self, W=None):
        w = np.ones(self.lb.shape[-1]) if W is None else np.asarray(W)
        return (self.lb * w.astype(np.longdouble)).T          # [P, nvox]

    def check(self, got, ref, log=False, what=""):
        """got [nvox] or [P, nvox] (float64, log10 already applied if `log`) against ref (longdouble, never logged)"""
        excluded = 1.0 - self.keep.mean()
        assert excluded <= EXCLUDED_MAX, f"{what}: {excluded:.0%} of the voxels have cond > {COND_MAX:g}"
        got = np.asarray(got)
        assert got.dtype == np.float64 and got.shape == ref.shape, (what, got.dtype, got.shape, ref.shape)
        if log:
            ref = np.log10(ref)
            err = np.abs(got - ref)
            bar = self.tol / np.log(10)
        else:
            err = np.abs(got - ref) / np.abs(ref)
            bar = self.tol
        err = np.where(self.keep, err.astype(np.float64), 0.0)
        ratio = float(np.max(err / bar))
        print(f"{what}: max err / tolerance = {ratio:.3g} (max err {float(err.max()):.3g}, cond up to "
              f"{float(self.cond[self.keep].max()):.3g}, {excluded:.0%} excluded)")
        assert np.all(np.isfinite(got[..., self.keep])), what
        assert ratio <= 1.0, (what, ratio)


def gaussian_records(seed, nrec, nprobe, nrow, nvox):
    """[nrec, nprobe, nrow, nvox] standard-normal complex entries"""
    rng = np.random.default_rng(seed)
    shape = (nrec, nprobe, nrow, nvox)
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def decaying_records(seed, nrec=1000, nvox=65):
    """[nrec, 1, 4, nvox]: exp(-3 t / T2) e^{i phi} times (1, 3 t / T2^2, sin(t / 3), cos(t / 5) + 0.01 noise), t = 0 .. nrec - 1,
    T2 uniform in 5 .. 200 per voxel -- columns like a signal and its derivatives over a 1000-TR train"""
    rng = np.random.default_rng(seed)
    T2 = rng.uniform(5.0, 200.0, nvox)
    phi = rng.uniform(0.0, 2 * np.pi, nvox)
    t = np.arange(nrec, dtype=np.float64)[:, None]
    base = np.exp(-3.0 * t / T2) * np.exp(1j * phi)
    noise = rng.standard_normal((nrec, nvox))
    cols = [np.ones_like(t) * np.ones(nvox), 3.0 * t / T2 ** 2, np.sin(t / 3.0) * np.ones(nvox), np.cos(t / 5.0) + 0.01 * noise]
    return np.stack([base * c for c in cols], axis=1)[:, None]


def columns(records, j, rows):
    """what the handle stands for: J [nvox, nrec, P] of probe j, columns `rows`"""
    return np.ascontiguousarray(np.moveaxis(records[:, j][:, list(rows)], (0, 1, 2), (1, 2, 0)))


def upload_jacobian(ctx, records, j, rows, grid=None):
    """the records in a DeviceBuffer, wrapped as the DeviceJacobian of probe j with columns `rows`"""
    from epgpy_amd import _lib, functions
    nrec, nprobe, nrow, nvox = records.shape
    buf = _lib.DeviceBuffer(ctx, records.nbytes)
    buf.upload(np.ascontiguousarray(records, dtype=np.complex128))
    grid = (nvox,) if grid is None else tuple(grid)
    return functions.DeviceJacobian(buf, nrec, grid, nprobe, nrow, j, list(rows), [f"v{r}" for r in rows])

"""Multi-compartment exchange, EPG-X (mirrors epgpy/exchange.py).

`X(tau, khi)` couples the N compartments of a voxel: the compartments are the N entries of one grid axis (`axis`), and
at every phase order the transverse and longitudinal states of the compartments mix through the matrix exponentials of
the kinetic matrix `khi` combined with relaxation and chemical shift (exchange.py:154-207).  With the plain equilibrium
[0, 0, rho] only Z_0 carries the affine term: Z_0 - rho is exchanged, then rho is added back (exchange.py:110-120).

Device form (include/epgx.h, EPGX_OP_X): one record with ia = N and ib = the compartment stride of the plan's grid;
one table entry per compartment GROUP (an index space with stride 0 on the compartment axis) of 3 N^2 doubles:
Re/Im of mT row-major, then mL row-major (real).
"""
import numpy as np

from . import common, operator, _lib

NAX = np.newaxis


class X(operator.Operator):
    """exchange between compartments, with relaxation and precession during `tau` (exchange.py:11-120)

    tau: mixing time (ms); khi: exchange rate (1/ms) between two compartments, or an N x N kinetic matrix (every column
    sums to 0 along `axis`); T1 / T2 (ms) and g (kHz, chemical shift) of the compartments along `axis`"""

    def __init__(self, tau, khi, *, axis=-1, T1=None, T2=None, g=None, name=None, duration=None):
        params = common.map_arrays(tau=tau, T1=T1, T2=T2, g=g)
        if common.isscalar(khi):      # a rate: two compartments (exchange.py:41-43)
            khi = exchange_matrix(khi, axis=axis, ncomp=2)
        else:                         # a kinetic matrix (exchange.py:44-57)
            khi = np.asarray(khi)
            if khi.ndim < 2:
                raise ValueError("Exchange matrix matrix must be at least 2D")
            if khi.shape[:-1][axis] != khi.shape[-1]:
                raise ValueError("Exchange matrix must be square")
            if not all(np.allclose(khi[..., i].sum(axis=axis), 0) for i in range(khi.shape[-1])):
                raise ValueError(f"Exchange matrix must sum to 0 along axis {axis}")
        axis = int(khi.ndim + axis - 1) if axis < 0 else int(axis)     # (exchange.py:59-60)

        self.axis = axis
        self.mat = exchange_operator(tau, khi, axis=axis, T1=T1, T2=T2, g=g)
        self.khi = khi
        self.T1, self.T2, self.g, self.tau = params["T1"], params["T2"], params["g"], params["tau"]
        self._duration = duration
        if duration is True:          # (exchange.py:76-79)
            duration = self.tau
        if name is None:
            name = common.repr_operator("X", ["tau", "khi"], [tau, khi])
        super().__init__(name=name, duration=duration)
        self._packed = None

    @property
    def shape(self):
        """mat.shape[:-1] without the second compartment axis (exchange.py:84-88)"""
        return tuple(d for i, d in enumerate(self.mat.shape[:-1]) if i != self.axis + 1)

    @property
    def ncomp(self):
        return self.mat.shape[self.axis]

    def _table(self):
        """[*shape with 1 on the compartment axis, 3 N^2]: Re/Im mT row-major, then mL row-major (real: its imaginary part is
        the rounding noise of the eigendecomposition, exchange.py:262-282)"""
        if self._packed is None:
            ax, n = self.axis, self.ncomp
            mT = np.moveaxis(self.mat[..., 0], (ax, ax + 1), (-2, -1))       # [*lead, N, N]
            mL = np.moveaxis(self.mat[..., 2], (ax, ax + 1), (-2, -1))
            lead = mT.shape[:-2]
            mT = np.stack([mT.real, mT.imag], axis=-1).reshape(lead + (2 * n * n,))
            tab = np.concatenate([mT, np.real(mL).reshape(lead + (n * n,))], axis=-1)
            self._packed = np.ascontiguousarray(np.expand_dims(tab, ax), dtype=np.float64)
        return self._packed

    def _encode(self, enc):
        n, ax = self.ncomp, self.axis
        enc.note_exchange(ax, n)
        stride = int(np.prod(enc.grid[ax + 1:]))
        enc.add(_lib.OP_X, table=self._table(), key=("X", id(self)), ia=n, ib=stride)
        enc.note("relax")

    def _apply(self, sm):
        """op(sm): states broadcast to the N compartments if sm has one along `axis`, conservation of the total
        magnetization checked against the densities of sm (exchange.py:89-108), then one launch"""
        if getattr(sm, "_eq", None) is not None:
            raise NotImplementedError("X on a state matrix with a general equilibrium")
        grid = common.broadcast_shapes(sm.shape, self.shape, append=True)
        sm._broadcast_to(grid)
        dens = np.asarray(sm.density, dtype=np.float64)
        dens = dens.reshape(dens.shape + (1,) * (len(grid) - dens.ndim))
        if not np.allclose(dotp(self.khi, dens[..., NAX], axes=[-1, self.axis]), 0):
            raise RuntimeError("Exchange matrix `khi` does not conserve total magnetization")
        return super()._apply(sm)


# ---------------------------------------------------------------------------------------------------------- functions


def exchange_matrix(k, *, axis=-1, ncomp=2, densities=None):
    """kinetic matrix of `ncomp` compartments exchanging at rate(s) `k` (exchange.py:127-151): off-diagonal entries
    -k / (ncomp - 1), diagonal k, optionally divided column-wise by `densities`; the two new axes of size ncomp sit at
    `axis` and at the end"""
    k = np.asarray(k)
    if np.any(k < 0):
        raise ValueError("Cannot have negative echange rate")
    if axis > k.ndim:
        k = np.expand_dims(k, tuple(range(k.ndim, axis)))
    axis = (k.ndim + axis + 1) if axis < 0 else axis
    kron = np.eye(ncomp) + (np.eye(ncomp) - 1) / (ncomp - 1)
    if densities is not None:
        kron = kron / densities
    return np.moveaxis(k[..., NAX, NAX] * kron, -2, axis)


def exchange_operator(tau, khi, *, axis=0, T1=None, T2=None, g=None):
    """[..., N, N, ..., 3] stack of (mT, conj mT, mL) acting on F+, F- and Z (exchange.py:154-207):
    mT = expm((-khi + (-1/T2 + 2 i pi g) I) tau), mL = expm((-khi - I / T1) tau)

    Van Landeghem M, Haber A, D'espinose De Lacaillerie J-B, Bluemich B.  Analysis of multisite 2D relaxation exchange NMR.
    Concepts Magn Reson 2010; 36A:153-169."""
    khi = np.asarray(khi)
    tau = np.asarray(tau)
    T1 = np.asarray(np.inf if T1 is None else T1)
    T2 = np.asarray(np.inf if T2 is None else T2)
    g = np.asarray(0 if g is None else g)
    eye = np.eye(khi.shape[-1])

    minshape = khi.shape[:-1]
    shape = _broadcast_shapes(tau.shape, T1.shape, T2.shape, g.shape, minshape)
    ndim = len(shape)
    tau, T1, T2, g = [np.expand_dims(a, tuple(range(a.ndim, ndim))) for a in (tau, T1, T2, g)]
    T1, T2, g = [np.broadcast_to(a, shape) for a in (T1, T2, g)]
    khi = np.expand_dims(khi, tuple(range(ndim - len(minshape))))
    tau, T1, T2, g = [np.moveaxis(a, axis, -1) for a in (tau, T1, T2, g)]   # compartments last

    xT = -khi + (-1 / T2 + 2j * np.pi * g)[..., NAX] * eye
    xL = -khi + (-1 / T1)[..., NAX] * eye
    mT = np.moveaxis(expm(xT * tau[..., NAX]), (-2, -1), (axis, axis + 1))
    mL = np.moveaxis(expm(xL * tau[..., NAX]), (-2, -1), (axis, axis + 1))
    return np.stack([mT, mT.conj(), mL], axis=-1)


def expm(mat):
    """matrix exponential through an eigendecomposition with expm1 (exchange.py:262-282); the same algorithm as the
    reference, so that the tables agree to rounding"""
    matnorm = np.linalg.norm(mat)
    if np.isclose(matnorm, 0):
        return np.eye(mat.shape[-1]).reshape(mat.shape)
    if np.allclose(mat, _transpose(mat).conj()):
        evals, evecs = np.linalg.eigh(mat / matnorm)
    else:
        evals, evecs = np.linalg.eig(mat / matnorm)
    eexp = np.expm1(evals * matnorm) + 1
    # V diag(e) V^-1, written as the solution of V^T Y = diag(e) V^T (no explicit inverse)
    return _transpose(np.linalg.solve(_transpose(evecs), eexp[..., NAX] * _transpose(evecs)))


def _broadcast_shapes(*shapes):
    """broadcast with trailing axes appended (shapes aligned on their first axis)"""
    return np.broadcast_shapes(*[shape[::-1] for shape in shapes])[::-1]


def _transpose(mat):
    return np.moveaxis(mat, -1, -2)


def dotp(a, b, axes=(-1, -1)):
    """sum over axis axes[0] of a times axis axes[1] of b (exchange.py:251-256)"""
    a, b = np.asarray(a), np.asarray(b)
    return np.einsum("...i,...i->...", np.moveaxis(a, axes[0], -1), np.moveaxis(b, axes[1], -1))

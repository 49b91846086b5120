"""Multi-compartment exchange, EPG-X (mirrors epgpy/exchange.py).

`X(tau, khi)` couples the N compartments of a voxel: the compartments are the N entries of one grid axis (`axis`), and
at every phase order the transverse and longitudinal states of the compartments mix through the matrix exponentials of
the kinetic matrix `khi` combined with relaxation and chemical shift (exchange.py:154-207).  With the plain equilibrium
[0, 0, rho] only Z_0 carries the affine term: Z_0 - rho is exchanged, then rho is added back (exchange.py:110-120).

Device form (include/epgx.h, EPGX_OP_X): one record with ia = N and ib = the compartment stride of the plan's grid;
one table entry per compartment GROUP (an index space with stride 0 on the compartment axis) of 3 N^2 doubles:
Re/Im of mT row-major, then mL row-major (real).

First-order derivatives (no counterpart in the reference, whose X is a plain Operator): `X(..., order1=...)` with the
parameters tau, khi, T1, T2, g.  `exchange_operator_partials` differentiates the two matrix exponentials (d/dtau = A m; the
others through the Frechet derivative of expm in the eigenbasis), and the operator ships one table per variable in the layout
of its own (d mT, d mL): dxrun_kernel (csrc/epgx_dxrun_kernels.hip.h) applies it to the state before the update.
"""
import numpy as np

from . import common, diff, operator, _lib

NAX = np.newaxis


class X(diff.DiffMixin, operator.Operator):
    """exchange between compartments, with relaxation and precession during `tau` (exchange.py:11-120)

    tau: mixing time (ms); khi: exchange rate (1/ms) between two compartments, or an N x N kinetic matrix (every column
    sums to 0 along `axis`); T1 / T2 (ms) and g (kHz, chemical shift) of the compartments along `axis`

    order1: first-order partials (DiffMixin forms) with respect to tau, khi, T1, T2, g.  T1 / T2 / g are per-compartment
    parameters: a scalar coefficient moves all compartments together, an array along the compartment axis weights them
    (`order1={"T2b": {"T2": [0, 1]}}`: the second compartment's T2).  "khi" differentiates along a direction in the space of
    kinetic matrices: for a scalar rate k, d khi / d k = exchange_matrix(1); for a kinetic matrix pass `dkhi=` (the shape
    of khi, e.g. exchange_matrix(1, densities=...)).  Densities do not depend on a variable"""

    PARAMETERS_ORDER1 = {"tau", "khi", "T1", "T2", "g"}

    def __init__(self, tau, khi, *, axis=-1, T1=None, T2=None, g=None, name=None, duration=None, dkhi=None, **kwargs):
        if kwargs.get("order2"):
            raise NotImplementedError("X (exchange): second-order derivatives (order2 / Hessian) are not supported")
        self._init_partials(kwargs)
        if kwargs:
            raise TypeError(f"X: unexpected keyword argument(s) {sorted(kwargs)}")
        params = common.map_arrays(tau=tau, T1=T1, T2=T2, g=g)
        if common.isscalar(khi):      # a rate: two compartments (exchange.py:41-43)
            if dkhi is None:
                dkhi = exchange_matrix(1.0, axis=axis, ncomp=2)
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

        if dkhi is not None:
            dkhi = np.asarray(dkhi, dtype=np.float64)
            if dkhi.shape != khi.shape:
                raise ValueError(f"dkhi must have the shape of khi: {dkhi.shape}, {khi.shape}")
        if "khi" in self.parameters_order1 and dkhi is None:
            raise ValueError("X: order1 names 'khi' of a kinetic matrix: pass its direction d khi / d variable as dkhi=")
        self.axis = axis
        self.mat = exchange_operator(tau, khi, axis=axis, T1=T1, T2=T2, g=g)
        self.khi = khi
        self.dkhi = dkhi
        self._args = (tau, T1, T2, g)
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

    @staticmethod
    def _pack(mT, mL, ax):
        """(mT, mL) [*shape with N, N at ax, ax + 1] -> [*shape with 1 on the compartment axis, 3 N^2]"""
        n = mT.shape[ax]
        mT, mL = np.moveaxis(mT, (ax, ax + 1), (-2, -1)), np.moveaxis(mL, (ax, ax + 1), (-2, -1))       # [*lead, N, N]
        lead = mT.shape[:-2]
        mT = np.stack([mT.real, mT.imag], axis=-1).reshape(lead + (2 * n * n,))
        tab = np.concatenate([mT, np.real(mL).reshape(lead + (n * n,))], axis=-1)
        return np.ascontiguousarray(np.expand_dims(tab, ax), dtype=np.float64)

    def _partial_tables(self, params):
        """{parameter: table}: tau / khi [*lead(1 at axis), 3 N^2]; T1 / T2 / g [N, *lead(1 at axis), 3 N^2], one table per
        compartment whose parameter moves"""
        tau, T1, T2, g = self._args
        partials = exchange_operator_partials(tau, self.khi, axis=self.axis, T1=T1, T2=T2, g=g, dkhi=self.dkhi, only=set(params))
        ax = self.axis
        out = {}
        for p, (dmT, dmL) in partials.items():
            if p in ("tau", "khi"):
                out[p] = self._pack(dmT, dmL, ax)
            else:
                out[p] = np.stack([self._pack(dmT[c], dmL[c], ax) for c in range(self.ncomp)])
        return out

    def _variable_tables(self):
        """{variable: [*shape with 1 on the compartment axis, 3 N^2] table of sum_p coeff * dX/dp}, memoised.  A non-scalar
        coefficient broadcasts against the operator's shape (trailing axes appended); along the compartment axis it weights
        the per-compartment partials of T1 / T2 / g"""
        if self._dtables is None:
            partials = self._partial_tables(self.parameters_order1)
            ax, n = self.axis, self.ncomp
            tables = {}
            for var, coeffs in self.order1.items():
                total = 0.0
                for param, coeff in coeffs.items():
                    coeff = np.asarray(coeff, dtype=np.float64)
                    tab = partials[param]
                    per_comp = param not in ("tau", "khi")
                    if coeff.ndim == 0:
                        total = total + float(coeff) * (tab.sum(axis=0) if per_comp else tab)
                        continue
                    ndim = max(tab.ndim - (2 if per_comp else 1), coeff.ndim)
                    coeff = coeff.reshape(coeff.shape + (1,) * (ndim - coeff.ndim))
                    if coeff.shape[ax] not in (1, n) or (not per_comp and coeff.shape[ax] != 1):
                        raise ValueError(f"X: coefficient of {param!r} has extent {coeff.shape[ax]} on the compartment axis {ax}")
                    pad = lambda t: t.reshape(t.shape[:-1] + (1,) * (ndim - (t.ndim - 1)) + t.shape[-1:])
                    if not per_comp:
                        total = total + pad(tab) * coeff[..., None]
                        continue
                    for c in range(n):
                        cc = np.take(coeff, [c if coeff.shape[ax] == n else 0], axis=ax)
                        total = total + pad(tab[c]) * cc[..., None]
                tables[var] = np.ascontiguousarray(total, dtype=np.float64)
            self._dtables = tables
        return self._dtables

    def _encode(self, enc):
        if getattr(enc, "hessian", None) is not None:
            raise NotImplementedError("X (exchange): second-order passes (Hessian) are not supported")
        n, ax = self.ncomp, self.axis
        enc.note_exchange(ax, n)
        stride = int(np.prod(enc.grid[ax + 1:]))
        enc.add(_lib.OP_X, table=self._table(), key=("X", id(self)), ia=n, ib=stride)
        if self.order1:
            enc.add_partials({var: ("entry", enc.partial_table(self, var)) for var in self.order1})
        enc.note("relax")

    def __call__(self, sm, *, inplace=False):
        if self.order1 or getattr(sm, "order1", None) or getattr(sm, "order2", None):
            raise NotImplementedError("X (exchange): derivative states run in simulate() only (one fused launch); op(sm) on a "
                                      "state matrix with order1 / order2, or of an X with order1, is not supported")
        return operator.Operator.__call__(self, sm, inplace=inplace)

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


def _generators(tau, khi, axis, T1, T2, g):
    """(A_T, A_L, tau, T1, T2, g) with the two compartment axes LAST ([..., N, N]; the parameters [..., N or 1]) as
    exchange_operator builds them: A_T = -khi + diag(-1/T2 + 2 i pi g), A_L = -khi - diag(1/T1); m = expm(A tau[..., None])"""
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
    return xT, xL, tau, T1, T2, g


def exchange_operator(tau, khi, *, axis=0, T1=None, T2=None, g=None):
    """[..., N, N, ..., 3] stack of (mT, conj mT, mL) acting on F+, F- and Z (exchange.py:154-207):
    mT = expm((-khi + (-1/T2 + 2 i pi g) I) tau), mL = expm((-khi - I / T1) tau)

    Van Landeghem M, Haber A, D'espinose De Lacaillerie J-B, Bluemich B.  Analysis of multisite 2D relaxation exchange NMR.
    Concepts Magn Reson 2010; 36A:153-169."""
    xT, xL, tau, _, _, _ = _generators(tau, khi, axis, T1, T2, g)
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


def expm_frechet(mat, direction):
    """Frechet derivative of the matrix exponential at `mat` [..., N, N] along `direction` (Daleckii-Krein, in the eigenbasis
    mat = V diag(lam) V^-1 of `expm`):  L = V [(V^-1 E V) o Phi] V^-1  with the divided differences of exp,
    Phi_ij = e^lam_j expm1(lam_i - lam_j) / (lam_i - lam_j) (evaluated with lam_j the eigenvalue of the larger real part),
    Phi_ii = e^lam_i -- also where two eigenvalues (nearly) coincide.
    (A block-triangular [[A, E], [0, A]] is defective: its eigendecomposition cannot serve.)"""
    mat = np.asarray(mat)
    direction = np.asarray(direction)
    if np.allclose(mat, _transpose(mat).conj()):
        evals, evecs = np.linalg.eigh(mat)
    else:
        evals, evecs = np.linalg.eig(mat)
    delta = evals[..., :, NAX] - evals[..., NAX, :]
    scale = np.maximum(np.abs(evals[..., :, NAX]), np.abs(evals[..., NAX, :]))
    same = np.abs(delta) <= FRECHET_EPS * np.maximum(scale, 1.0)
    # the divided difference is symmetric in (i, j): factor out the eigenvalue with the LARGER real part, so that expm1 sees a
    # difference with a non-positive real part.  The other orientation multiplies e^lam_small by expm1(+|delta|), two factors whose
    # relative errors (|lam| eps each, from the rounding of the eigenvalues) do not cancel: 500 eps for a bound pool's T2 of 10 us
    swap = delta.real > 0                                   # lam_i is the larger one: e^lam_i expm1(lam_j - lam_i) / (lam_j - lam_i)
    safe = np.where(same, 1.0, np.where(swap, -delta, delta))
    base = np.where(swap, np.exp(evals)[..., :, NAX] + 0 * delta, np.exp(evals)[..., NAX, :] + 0 * delta)
    phi = np.where(same, np.exp(evals)[..., :, NAX] + 0 * delta, base * np.expm1(safe) / safe)
    inner = np.linalg.solve(evecs, direction @ evecs) * phi                      # (V^-1 E V) o Phi
    return _transpose(np.linalg.solve(_transpose(evecs), _transpose(evecs @ inner)))   # V inner V^-1


FRECHET_EPS = 1e-14     # |lam_i - lam_j| below this (relative to max(1, |lam|)): the limit e^lam_i (error <= 5e-15 relative)


def exchange_operator_partials(tau, khi, *, axis=0, T1=None, T2=None, g=None, dkhi=None, only=None):
    """partial derivatives of `exchange_operator`: {parameter: (d mT, d mL)} in its layout ([..., N, N, ...], the compartment
    axes at `axis`, `axis + 1`).  "tau" and "khi" give one pair; "T1", "T2", "g" are per-compartment parameters and give
    [N, ...] stacks: entry c differentiates with respect to the parameter of compartment c (their sum: all compartments
    together).  "khi" differentiates along `dkhi` (the shape of khi; required for it).  `only`: the parameters wanted.

    d/dtau = A m (A and m commute); the others are Frechet derivatives of expm along E = tau dA/dp:
    dA_T/dT2_c = +1/T2_c^2 and dA_T/dg_c = 2 i pi at (c, c), dA_L/dT1_c = +1/T1_c^2 at (c, c), dA/dk = -dkhi."""
    want = (lambda name: True) if only is None else (lambda name: name in only)
    xT, xL, tau_, T1_, T2_, g_ = _generators(tau, khi, axis, T1, T2, g)
    n = xT.shape[-1]
    aT, aL = xT * tau_[..., NAX], xL * tau_[..., NAX]
    place = lambda m: np.moveaxis(m, (-2, -1), (axis, axis + 1))
    shape = np.broadcast_shapes(aT.shape, aL.shape)
    full = lambda m: np.broadcast_to(m, shape)
    out = {}
    if want("tau"):
        if tau_.shape[-1] != 1:
            raise NotImplementedError("X: d/dtau with a mixing time that varies along the compartment axis")
        out["tau"] = (place(full(xT @ expm(aT))), place(full(np.real(xL @ expm(aL)))))
    if want("khi"):
        if dkhi is None:
            raise ValueError("exchange_operator_partials: 'khi' needs its direction dkhi= (the shape of khi)")
        dk = np.asarray(dkhi, dtype=np.float64)
        dk = np.expand_dims(dk, tuple(range(xT.ndim - dk.ndim)))
        e = -dk * tau_[..., NAX]
        out["khi"] = (place(full(expm_frechet(aT, e + 0 * aT))), place(full(np.real(expm_frechet(aL, e + 0 * aL)))))
    unit = lambda c: np.eye(n)[c][:, NAX] * np.eye(n)[c][NAX, :]          # the (c, c) unit matrix
    zero = np.zeros(shape)
    with np.errstate(divide="ignore"):
        rates = {"T2": (1 / T2_ ** 2, True), "g": (2j * np.pi + 0 * g_, True), "T1": (1 / T1_ ** 2, False)}
    for p, (rate, transverse) in rates.items():
        if not want(p):
            continue
        rate = np.broadcast_to(rate, np.broadcast_shapes(rate.shape, shape[:-1]))
        parts = []
        for c in range(n):
            e = (rate[..., c] * tau_[..., 0 if tau_.shape[-1] == 1 else c])[..., NAX, NAX] * unit(c)
            a = aT if transverse else aL
            d = full(expm_frechet(a, e + 0 * a))
            parts.append((place(d), place(zero)) if transverse else (place(zero), place(np.real(d))))
        out[p] = (np.stack([t for t, _ in parts]), np.stack([l for _, l in parts]))
    return out


def _broadcast_shapes(*shapes):
    """broadcast with trailing axes appended (shapes aligned on their first axis)"""
    return np.broadcast_shapes(*[shape[::-1] for shape in shapes])[::-1]


def _transpose(mat):
    return np.moveaxis(mat, -1, -2)


def dotp(a, b, axes=(-1, -1)):
    """sum over axis axes[0] of a times axis axes[1] of b (exchange.py:251-256)"""
    a, b = np.asarray(a), np.asarray(b)
    return np.einsum("...i,...i->...", np.moveaxis(a, axes[0], -1), np.moveaxis(b, axes[1], -1))

"""Cases and the yardstick of `epgpy_amd.match.nnls`, shared by tests/test_nnls_host.py (CPU) and tests/test_gpu_nnls.py.

The yardstick evaluates, in numpy.longdouble and from the RAW dictionary and signals (no Gram matrix), what the definition of
`nnls` is about, for any given weights x of a voxel in a group:

    J(x)  = sum_t |S[t,m] - sum_a x_a D[t,a,g]|^2 + mu_g |x|^2         mu_g = reg * mean over the valid atoms of sum_t |D[t,a,g]|^2
    w_a   = Re sum_t conj(D[t,a,g]) (S[t,m] - sum_b x_b D[t,b,g]) - mu_g x_a      (the KKT quantities: minus half the gradient)

The reference is `scipy.optimize.nnls` on the stacked real system [Re D; Im D; sqrt(mu) I] x ~ [Re S; Im S; 0].

MARGIN, the relative amount by which J of the code under test may exceed J of scipy (and, for `nnls_host`, the other way round).
Two minimisers of a strictly convex quadratic that end on the same passive set differ in J by dx^T (H + mu I) dx, of second
order in the error dx of the passive-set solve.  Along the eigenvector of eigenvalue lambda_i the Gram-form solve errs by about
u lambda_max |x| / lambda_i (u = 2^-53), which costs lambda_i (u lambda_max |x| / lambda_i)^2 <= u^2 cond lambda_max |x|^2 per
direction.  With the ridge cond(H + mu I) <= A / reg, lambda_max |x|^2 is of the order of A E, and the noise of the regular cases
keeps J at or above 1e-4 E: at the very worst (A = 64 directions, reg = 1e-8) that is 64 * 1.2e-32 * 6.4e9 * 64 / 1e-4 = 3e-15
relative to J.  MEASURED between `nnls_host` and scipy 1.15 over every regular case, either way round: at most 5.1e-18
(tests/test_nnls_host.py prints it per case), which is the resolution of the longdouble yardstick itself (2^-64 = 5.4e-20 per
operation, sums of up to 64 x 80 terms of the size of the signal against a residual of 1e-2 of it).  MARGIN = 1e-12 stands
three orders above the worst case of the bound and is still far below the cost of a wrong passive set: an atom that should
carry weight x_a and does not costs about x_a^2 H_aa (1 - cos^2) >= 1e-6 J in these cases.

WEIGHT_TOL(cond): where reg >= 1e-4 both solutions solve the same well-posed problem and the weights agree within
cond(H + mu I) * 2^-53 * 64 * max|x| (the forward error of a Cholesky solve, 64 for the sums of up to 64 terms), doubled for the two
solutions compared.

RESIDUAL_TOL(nrec, A, E): `residual` is the root of J - mu |x|^2 taken from the Gram form, J = E - sum_a x_a (f_a + w_a).  E and every
f_a are sums of 2 nrec products, the sum over a has up to A terms of total size about E, and w_a on the passive set is a
difference of up to A terms of the size of f_a: |dJ| <= 8 (nrec + A) 2^-53 E.  Two roots whose squares differ by dJ differ by at
most sqrt(|dJ|), which is the bound -- about 4e-7 sqrt(E) at nrec + A = 144; the Gram form cannot do better near a residual of 0."""
import numpy as np

LD = np.longdouble
MARGIN = 1e-12


def split(D, axis):
    """D [nrec, *grid] -> [nrec, A, G]: the component axis out, every other axis flattened in C order"""
    nrec, grid = D.shape[0], D.shape[1:]
    axis = axis % len(grid)
    nouter = int(np.prod(grid[:axis], dtype=np.int64))
    ninner = int(np.prod(grid[axis + 1:], dtype=np.int64))
    return np.moveaxis(D.reshape(nrec, nouter, grid[axis], ninner), 2, 1).reshape(nrec, grid[axis], nouter * ninner)


class Yardstick:
    """J and the KKT quantities in longdouble from the raw D [nrec, *grid], S [nrec, nmeas]"""

    def __init__(self, D, S, axis, reg):
        self.D = split(np.asarray(D, dtype=np.complex128), axis)
        self.S = np.asarray(S, dtype=np.complex128).reshape(self.D.shape[0], -1)
        self.reg = reg
        self.nrec, self.A, self.G = self.D.shape
        with np.errstate(all="ignore"):
            n = (self.D.real.astype(LD) ** 2 + self.D.imag.astype(LD) ** 2).sum(axis=0)          # [A, G]
        self.valid = np.isfinite(n) & (n > 0)
        self.norms = n
        self.mu = np.array([LD(reg) * n[self.valid[:, g], g].sum() / max(self.valid[:, g].sum(), 1) for g in range(self.G)], dtype=LD)

    def _parts(self, m, g, x):
        ok = self.valid[:, g]
        d = self.D[:, ok, g]
        dr, di = d.real.astype(LD), d.imag.astype(LD)
        xv = np.asarray(x, dtype=LD)[ok]
        rr = self.S[:, m].real.astype(LD) - dr @ xv
        ri = self.S[:, m].imag.astype(LD) - di @ xv
        return ok, dr, di, xv, rr, ri

    def J(self, m, g, x):
        """the objective of voxel m in group g at the weights x [A] (invalid atoms must carry 0)"""
        ok, _, _, xv, rr, ri = self._parts(m, g, x)
        assert np.all(np.asarray(x)[~ok] == 0)
        return (rr ** 2).sum() + (ri ** 2).sum() + self.mu[g] * (xv ** 2).sum()

    def residual(self, m, g, x):
        _, _, _, _, rr, ri = self._parts(m, g, x)
        return np.sqrt((rr ** 2).sum() + (ri ** 2).sum())

    def kkt(self, m, g, x):
        """w [A] (0 for invalid atoms) and the scale sqrt(n_a E) it is measured on"""
        ok, dr, di, xv, rr, ri = self._parts(m, g, x)
        w = np.zeros(self.A, dtype=LD)
        w[ok] = dr.T @ rr + di.T @ ri - self.mu[g] * xv
        E = (self.S[:, m].real.astype(LD) ** 2 + self.S[:, m].imag.astype(LD) ** 2).sum()
        return w, np.sqrt(np.where(ok, self.norms[:, g], 0) * E)

    def energy(self, m):
        return float((self.S[:, m].real.astype(LD) ** 2 + self.S[:, m].imag.astype(LD) ** 2).sum())


def scipy_reference(D, S, axis, reg):
    """scipy.optimize.nnls on the stacked real system of every (voxel, group): weights [G, A, nmeas] (0 for invalid atoms)"""
    from scipy.optimize import nnls
    Dg = split(np.asarray(D, dtype=np.complex128), axis)
    S = np.asarray(S, dtype=np.complex128).reshape(Dg.shape[0], -1)
    nrec, A, G = Dg.shape
    out = np.zeros((G, A, S.shape[1]))
    for g in range(G):
        with np.errstate(all="ignore"):
            n = (np.abs(Dg[:, :, g]) ** 2).sum(axis=0)
        ok = np.isfinite(n) & (n > 0)
        if not ok.any():
            continue
        mu = reg * n[ok].sum() / ok.sum()
        d = Dg[:, ok, g]
        M = np.concatenate([d.real, d.imag, np.sqrt(mu) * np.eye(int(ok.sum()))], axis=0)
        for m in range(S.shape[1]):
            rhs = np.concatenate([S[:, m].real, S[:, m].imag, np.zeros(int(ok.sum()))])
            out[g, ok, m] = nnls(M, rhs, maxiter=30 * A)[0]
    return out


def cond_ridge(D, axis, reg):
    """cond_2(H_g + mu_g I) of every group, over the valid atoms"""
    Dg = split(np.asarray(D, dtype=np.complex128), axis)
    out = []
    for g in range(Dg.shape[2]):
        d = Dg[:, :, g]
        H = (np.conj(d).T @ d).real
        mu = reg * np.trace(H) / H.shape[0]
        out.append(np.linalg.cond(H + mu * np.eye(H.shape[0])))
    return np.array(out)


def residual_tol(nrec, A, E):
    return np.sqrt(8 * (nrec + A) * 2.0 ** -53 * E)


def weight_tol(cond, x):
    return 2 * 64 * cond * 2.0 ** -53 * np.max(np.abs(x))


# ---------------------------------------------------------------------------------------------------------------- dictionaries
def decay_dictionary(rng, nrec, grid, axis, phase=True):
    """echo-train-like atoms: exp(-(t + 1) r_a) along the component axis, modulated per group by an alternating, decaying
    term (what a B1 error does to the odd and even echoes), times one common phase"""
    A = grid[axis]
    rate = np.geomspace(0.02, 1.5, A) if A > 1 else np.array([0.2])
    t = np.arange(1, nrec + 1, dtype=np.float64)
    atoms = np.exp(-t[:, None] * rate[None, :])                                 # [nrec, A]
    other = [n for i, n in enumerate(grid) if i != axis]
    G = int(np.prod(other, dtype=np.int64))
    mod = 1.0 + 0.35 * ((np.arange(G) + 1.0) / G)[None, :] * ((-1.0) ** t * np.exp(-0.15 * t))[:, None]      # [nrec, G]
    D = atoms[:, :, None] * mod[:, None, :]                                      # [nrec, A, G]
    D = np.moveaxis(D.reshape((nrec, A) + tuple(other)), 1, 1 + axis)
    if phase:
        D = D * np.exp(1j * 0.7)
    return np.ascontiguousarray(D.astype(np.complex128))


def gauss_dictionary(rng, nrec, grid, phase=True):
    D = rng.standard_normal((nrec,) + tuple(grid))
    if phase:
        D = D + 1j * rng.standard_normal(D.shape)
    return np.ascontiguousarray(D.astype(np.complex128))


def mixtures(rng, D, axis, nmeas, noise, sparse=3):
    """signals: in a random group, `sparse` atoms (all of them for sparse = 0) with weights in [0.2, 1.2], plus complex noise of
    `noise` times the rms of the clean signal; returns S [nrec, nmeas] and the groups"""
    Dg = split(D, axis)
    nrec, A, G = Dg.shape
    grp = rng.integers(0, G, nmeas)
    S = np.empty((nrec, nmeas), dtype=np.complex128)
    for m in range(nmeas):
        x = np.zeros(A)
        on = rng.choice(A, size=min(sparse, A), replace=False) if sparse else np.arange(A)
        x[on] = 0.2 + rng.random(len(on))
        clean = Dg[:, :, grp[m]] @ x
        rms = np.sqrt(np.mean(np.abs(clean) ** 2))
        e = rng.standard_normal(nrec) + (1j * rng.standard_normal(nrec) if np.iscomplexobj(D) and np.abs(D.imag).max() > 0 else 0)
        S[:, m] = clean + noise * rms * e
    return S, grp


def cases():
    """name -> dict(D [nrec, *grid], S [nrec, nmeas], axis, reg): the regular cases.  Every one must come back with status 0 on
    every voxel (tests/test_nnls_host.py shows that `nnls_host` does)"""
    out = {}

    def add(name, D, axis, nmeas, reg, noise=0.02, sparse=3, seed=0):
        rng = np.random.default_rng(seed)
        S, grp = mixtures(rng, D, axis, nmeas, noise, sparse)
        out[name] = dict(D=D, S=S, axis=axis, reg=reg, truth=grp)

    rng = np.random.default_rng(1)
    add("a1_r1_g1_m1", decay_dictionary(rng, 1, (1,), 0), 0, 1, 1e-8)
    add("a3_r8_g3_m65", decay_dictionary(rng, 8, (3, 3), 0), 0, 65, 1e-8)
    add("a33_r33_g3_m130", decay_dictionary(rng, 33, (33, 3), 0), 0, 130, 1e-8)
    add("a40_r33_g1_m65_real", decay_dictionary(rng, 33, (40,), 0, phase=False), 0, 65, 1e-4)
    add("a64_r33_g3_m65", decay_dictionary(rng, 33, (3, 64), 1), 1, 65, 1e-4)
    add("a33_r8_g1_m130", decay_dictionary(rng, 8, (33,), 0), 0, 130, 1e-6)
    add("a40_r1_g3_m65", gauss_dictionary(rng, 1, (40, 3)), 0, 65, 1e-2)
    add("full_a64_r80_g1_m9", gauss_dictionary(rng, 80, (64,)), 0, 9, 1e-2, noise=0.01, sparse=0)
    add("full_a40_r48_g3_m1", gauss_dictionary(rng, 48, (3, 40)), 1, 1, 1e-2, noise=0.01, sparse=0)
    add("reg0_a8_r33_g3_m65_real", gauss_dictionary(rng, 33, (8, 3), phase=False), 0, 65, 0.0, noise=0.1)
    add("axis_first", decay_dictionary(rng, 8, (5, 3, 2), 0), 0, 65, 1e-8)
    add("axis_middle", decay_dictionary(rng, 8, (3, 5, 2), 1), 1, 65, 1e-8)
    add("axis_last", decay_dictionary(rng, 8, (3, 2, 5), 2), 2, 65, 1e-8)
    return out


def special():
    """the degenerate dictionary: grid (6, 4), component axis 0.  Group 0 regular; group 1 with atom 2 holding a NaN and atom 4
    all zero; group 2 with every atom invalid (zeros and a NaN); group 3 a copy of group 0.  Signals: 0 all zero, 1 .. 3 mixtures
    of group 1's valid atoms, 4 .. 6 mixtures of group 0"""
    rng = np.random.default_rng(7)
    D = decay_dictionary(rng, 8, (6, 4), 0)
    D[:, 2, 1] = np.nan
    D[:, 4, 1] = 0.0
    D[:, :, 2] = 0.0
    D[3, 1, 2] = np.nan
    D[:, :, 3] = D[:, :, 0]
    S = np.zeros((8, 7), dtype=np.complex128)
    for m in (1, 2, 3):
        S[:, m] = D[:, [0, 1, 3, 5], 1] @ (0.3 + rng.random(4)) + 0.01 * (rng.standard_normal(8) + 1j * rng.standard_normal(8))
    for m in (4, 5, 6):
        S[:, m] = D[:, :, 0] @ (0.3 + rng.random(6)) + 0.01 * (rng.standard_normal(8) + 1j * rng.standard_normal(8))
    return dict(D=D, S=S, axis=0, reg=1e-6)

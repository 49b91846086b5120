"""Cases and references of the chi^2-driven ridge of `epgpy_amd.match.nnls(..., chi2=)`, shared by tests/test_nnls_chi2_host.py
(CPU) and tests/test_gpu_nnls_chi2.py.  The yardstick, MARGIN, residual_tol and the dictionary makers are those of
tests/nnls_cases.py; everything here is evaluated in numpy.longdouble from the RAW dictionary and signals (no Gram matrix):

    Jd(x)     = sum_t |S[t,m] - sum_a x_a D[t,a,g]|^2                      the data misfit
    J(x; mu)  = Jd(x) + mu |x|^2                                           the objective at an ABSOLUTE ridge mu (the device's own)

The reference is `scipy.optimize.nnls` on the stacked real system [Re D; Im D; sqrt(mu) I] inside `scipy.optimize.brentq` on
log mu: bracketed from mu_0 upward by factors of 16, it must reach |Jd / (chi2 Jd_0) - 1| <= chi2_rtol on its own.

GRAM(nrec, A, E) = 8 (nrec + A) 2^-53 E is the documented rounding of the Gram-form J (tests/nnls_cases.py, RESIDUAL_TOL): the
chi^2 condition is met by the code under test in the Gram form, so in extended precision it holds within chi2_rtol plus that
rounding of the two misfits over Jd_0.

The shapes are the smallest at which the lanes, the LDS triangle and the search can go wrong: A in {1, 3, 5, 33, 64} (1 is a
scalar, 64 fills the wavefront), nrec in {8, 33, 48}, G in {1, 3} with the component axis first, in the middle and last, nmeas in
{1, 9, 65, 130}, a decay and a Gauss dictionary, real and with a common phase, noise 0.02 and 0.002, chi2 in {1.02, 1.5}."""
import numpy as np

from tests import nnls_cases as nc

LD = nc.LD
RTOL = 1e-3           # the default chi2_rtol
FACTOR = 16.0         # the step of the bracket (NNLS_CHI2_FACTOR)
EVALS = 40            # the cap of a voxel's search (NNLS_CHI2_EVALS)


def gram_rounding(nrec, A, E):
    return 8 * (nrec + A) * 2.0 ** -53 * E


def misfit(y, m, g, x):
    """Jd(x) of voxel m in group g, longdouble"""
    return y.residual(m, g, x) ** 2


def objective(y, m, g, x, mu):
    """J(x; mu) at the absolute ridge mu, longdouble"""
    return misfit(y, m, g, x) + LD(mu) * (np.asarray(x, dtype=LD) ** 2).sum()


def scipy_at(y, m, g, mu):
    """scipy's weights of voxel m in group g at the absolute ridge mu, on the stacked real system"""
    from scipy.optimize import nnls
    ok = y.valid[:, g]
    d = y.D[:, ok, g]
    M = np.concatenate([d.real, d.imag, np.sqrt(float(mu)) * np.eye(int(ok.sum()))], axis=0)
    rhs = np.concatenate([y.S[:, m].real, y.S[:, m].imag, np.zeros(int(ok.sum()))])
    out = np.zeros(y.A)
    out[ok] = nnls(M, rhs, maxiter=30 * y.A)[0]
    return out


def scipy_brentq(y, m, g, chi2):
    """the reference search: (mu, x, Jd / (chi2 Jd_0) - 1) with brentq on log mu from the bracket [mu_0 16^(j-1), mu_0 16^j]"""
    from scipy.optimize import brentq
    mu0 = float(y.mu[g])
    T = chi2 * misfit(y, m, g, scipy_at(y, m, g, mu0))

    def r(t):
        return float(misfit(y, m, g, scipy_at(y, m, g, np.exp(t))) / T - 1)

    lo = np.log(mu0)
    hi = lo + np.log(FACTOR)
    while r(hi) < 0:
        lo, hi = hi, hi + np.log(FACTOR)
    t = brentq(r, lo, hi, xtol=1e-12, rtol=1e-14)
    return np.exp(t), scipy_at(y, m, g, np.exp(t)), r(t)


def cases():
    """name -> dict(D, S, axis, reg, chi2): the regular cases.  Every voxel of every one must come back with status 0
    (tests/test_nnls_chi2_host.py shows that `nnls_host` does, and that the reference reaches the condition)"""
    out = {}

    def add(name, D, axis, nmeas, chi2, noise, sparse=2, seed=0):
        rng = np.random.default_rng(seed)
        S, grp = nc.mixtures(rng, D, axis, nmeas, noise, sparse)
        out[name] = dict(D=D, S=S, axis=axis, reg=1e-8, chi2=chi2, truth=grp, decay=not name.startswith("gauss"))

    rng = np.random.default_rng(11)
    add("a1_r8_g1_m1", nc.decay_dictionary(rng, 8, (1,), 0), 0, 1, 1.02, 0.02)
    add("a3_r8_g3_m130", nc.decay_dictionary(rng, 8, (3, 3), 0), 0, 130, 1.5, 0.02, sparse=1)
    add("a33_r33_g3_m65", nc.decay_dictionary(rng, 33, (33, 3), 0), 0, 65, 1.02, 0.002)
    add("a64_r48_g1_m9_real", nc.decay_dictionary(rng, 48, (64,), 0, phase=False), 0, 9, 1.02, 0.02)
    add("a64_r33_g3_m9", nc.decay_dictionary(rng, 33, (3, 64), 1), 1, 9, 1.5, 0.002)
    add("gauss_a33_r48_g1_m9", nc.gauss_dictionary(rng, 48, (33,)), 0, 9, 1.02, 0.02)
    add("gauss_a3_r8_g3_m65_real", nc.gauss_dictionary(rng, 8, (3, 3), phase=False), 0, 65, 1.5, 0.002)
    add("axis_first", nc.decay_dictionary(rng, 8, (5, 1, 3), 0), 0, 9, 1.02, 0.02)
    add("axis_middle", nc.decay_dictionary(rng, 8, (3, 5, 1), 1), 1, 65, 1.02, 0.002)
    add("axis_last", nc.decay_dictionary(rng, 8, (1, 3, 5), 2), 2, 9, 1.5, 0.02)
    return out


def edge():
    """the voxels of statuses 3 and 4 on a decay dictionary of 6 atoms, 8 records, one group (real, so that an imaginary signal is
    orthogonal to every atom): 0 a noise-free multiple of one atom (its misfit is the bias of the ridge, 1e-16 E: status 4), 1 a signal orthogonal to every atom (T >= E: status 3),
    2 a weak fit -- a mixture drowned in an orthogonal part, whose misfit chi2 = 1.5 cannot grow by half (status 3), 3 a regular
    noisy mixture, 4 all zero (status 4)"""
    rng = np.random.default_rng(13)
    D = nc.decay_dictionary(rng, 8, (6,), 0, phase=False)
    S = np.zeros((8, 5), dtype=np.complex128)
    S[:, 0] = 0.7 * D[:, 1]
    S[:, 1] = 1j * rng.standard_normal(8)
    S[:, 2] = D[:, [1, 4]] @ np.array([0.7, 0.4]) + 3j * rng.standard_normal(8)
    S[:, 3] = D[:, [1, 4]] @ np.array([0.7, 0.4]) + 0.02 * rng.standard_normal(8)
    return dict(D=D, S=S, axis=0, reg=1e-8, chi2=1.5)

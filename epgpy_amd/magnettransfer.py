"""Magnetization transfer: saturation and absorption rates of a bound pool (mirrors epgpy/magnettransfer.py).

Host arithmetic only.  In a sequence, MT is a two-pool exchange `X` with the bound pool kept out of the rotations
(`T([alpha, 0], phi)`), saturated by a relaxation-only operator `R(rL=[0, W])` with W from `saturation_rate`, and the
pools summed by `Adc(reduce=<compartment axis>)`.
"""
import numpy as np

from . import utils

NAX = np.newaxis


def _trapezoid(y, x=None, dx=1.0, axis=-1):
    trapz = getattr(np, "trapezoid", None) or np.trapz
    return trapz(y, x=x, dx=dx, axis=axis)


def saturation_rate(duration, rf, G, *, gamma=utils.gamma_1H):
    """saturation rate (1/ms) of the bound pool under an RF pulse (magnettransfer.py:22-51); valid while the pulse's
    bandwidth is much smaller than that of the bound pool

    duration: pulse duration (ms); rf: amplitude (uT) of a hard pulse, or a waveform sampled uniformly over `duration`;
    G: absorption line value of the bound pool at the pulse's offset (ms); gamma: gyromagnetic ratio (kHz/T)

    Graham SJ, Henkelman RM.  Understanding pulsed magnetization transfer.  J Magn Reson Imaging 1997; 7:903-912."""
    if np.isscalar(rf):
        integral = duration * rf**2
    else:
        rf = np.asarray(rf)
        integral = _trapezoid(rf**2, dx=duration / (len(rf) - 1))
    # W = pi gamma^2 G <B1^2>, in SI units (gamma in rad/s/T, B1 in T, G in s), then per ms
    W = np.pi * (1e-3 * 2 * np.pi * gamma) ** 2 * (1e-3 * G) * integral / duration
    return W * 1e-3


def absorption_rate(T2, lineshape, offres=0):
    """absorption line value G of the bound pool at `offres` (kHz) for its T2 (ms) (magnettransfer.py:54-112), returned in
    the reference's units (G / 1000); lineshape: 'gaussian', 'lorentzian' or 'super-lorentzian'.  The super-Lorentzian
    integrand is singular at the magic angle: below 1 kHz the line is a cubic spline through its values at +-1 .. 11 kHz.

    Morrison C, Stanisz G, Henkelman RM.  Modeling magnetization transfer for biological-like systems using a semi-solid
    pool with a super-Lorentzian lineshape and dipolar reservoir.  J Magn Reson B 1995; 108:103-113.
    Gloor M, Scheffler K, Bieri O.  Quantitative magnetization transfer imaging using balanced SSFP.  Magn Reson Med 2008;
    60:691-700."""
    offres = np.asarray(offres)
    x = 2 * np.pi * T2 * offres
    if lineshape == "gaussian":
        G = T2 / (2 * np.pi) ** 0.5 * np.exp(-(x**2) / 2)
    elif lineshape == "lorentzian":
        G = T2 / np.pi / (1 + x**2)
    elif lineshape == "super-lorentzian":
        u = np.linspace(0, 1, 1000).reshape([1] * x.ndim + [-1])

        def line(xs):       # integral over u = cos(theta) of the super-Lorentzian kernel
            d = 3 * u**2 - 1
            return T2 * (2 / np.pi) ** 0.5 * _trapezoid(1 / np.abs(d) * np.exp(-2 * (xs[..., NAX] / d) ** 2), u, axis=-1)

        G = np.zeros(offres.shape)
        valid = np.abs(offres) >= 1
        G[valid] = line(x[valid])
        knots = 2 * np.pi * T2 * np.array([1, 3, 5, 7, 9, 11])
        Gk = line(knots)
        G[~valid] = cubic_interp1d(x[~valid], np.r_[-knots[::-1], knots], np.r_[Gk[::-1], Gk])
    else:
        raise ValueError(f"Unknown lineshape: {lineshape}")
    return G * 1e-3


def cubic_interp1d(x0, x, y):
    """natural cubic spline through (x, y), evaluated at x0 (magnettransfer.py:115-190): the tridiagonal system of the
    second derivatives solved through its Cholesky factor (a bidiagonal matrix: two sweeps)"""
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    if np.any(np.diff(x) < 0):
        order = np.argsort(x)
        x, y = x[order], y[order]
    n = len(x)
    h, dy = np.diff(x), np.diff(y)

    diag = np.empty(n)       # L's diagonal
    sub = np.empty(n - 1)    # L's sub-diagonal
    z = np.empty(n)
    diag[0] = np.sqrt(2 * h[0])
    sub[0] = 0.0
    z[0] = 0.0 / diag[0]     # natural end condition
    for i in range(1, n - 1):
        sub[i] = h[i - 1] / diag[i - 1]
        diag[i] = np.sqrt(2 * (h[i - 1] + h[i]) - sub[i - 1] * sub[i - 1])
        rhs = 6 * (dy[i] / h[i] - dy[i - 1] / h[i - 1])
        z[i] = (rhs - sub[i - 1] * z[i - 1]) / diag[i]
    i = n - 1
    sub[i - 1] = h[-1] / diag[i - 1]
    diag[i] = np.sqrt(2 * h[-1] - sub[i - 1] * sub[i - 1])
    z[i] = (0.0 - sub[i - 1] * z[i - 1]) / diag[i]
    # back substitution with L^T
    z[i] = z[i] / diag[i]
    for i in range(n - 2, -1, -1):
        z[i] = (z[i] - sub[i - 1] * z[i + 1]) / diag[i]

    index = np.clip(x.searchsorted(x0), 1, n - 1)
    x1, xl = x[index], x[index - 1]
    y1, yl = y[index], y[index - 1]
    z1, zl = z[index], z[index - 1]
    hi = x1 - xl
    return (zl / (6 * hi) * (x1 - x0) ** 3 + z1 / (6 * hi) * (x0 - xl) ** 3
            + (y1 / hi - z1 * hi / 6) * (x0 - xl) + (yl / hi - zl * hi / 6) * (x1 - x0))

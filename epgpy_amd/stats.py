"""Statistics behind the Jacobians: Cramer-Rao lower bounds and delta-method confidence intervals, with the names, argument
meaning and return shapes of the reference (epgpy/stats.py).

Two kinds of input:

* **A `DeviceJacobian`** (`simulate(..., probe=epg.Jacobian([...]), out="device")`): the records stay in HBM and
  `crlb` / `crlb_split` run `crlb_kernel` on them (csrc/epgx_stats.hip through `epgx_signal_crlb`) -- every Jacobian byte is read
  once on the device and only the map, 8 bytes per voxel (and column for `crlb_split`), crosses PCIe.  The records of the
  handle (its axis 0) are the points: `crlb(jac_dev, ...)` is `crlb(np.moveaxis(np.asarray(jac_dev), 0, -2), ...)`.
  This path takes `W` as a vector of `nparam` values (or None) and a scalar `sigma2`; `H`, a `W` / `sigma2` that varies over the
  grid and handles of a run over several GPUs raise `NotImplementedError` naming the argument.
  With a `DeviceHessian` next to it (`simulate(..., probe=epg.Hessian(params, design), mode="resident", out="device")`)
  `crlb_grad` returns the cost and its gradient with respect to the design variables: `crlb_grad_kernel` through
  `epgx_signal_crlb_grad` reads both where they lie, and 8 (1 + nx) bytes per voxel cross PCIe.
* **A NumPy array** `[..., npoint, nparam]` the caller already holds: the reference's formulas in NumPy, any `nparam`, `H`
  included.  Post-processing on the host, like `utils.imaging` -- not a CPU path of the simulation.

Singular voxels.  The reference sets the information matrix to NaN where `cond(I) > 1e30`, which in float64 means exactly or
almost exactly singular.  The host branch does the same.  The device reports NaN for a voxel (in every row of `crlb_split`)
whenever a Cholesky pivot of its information matrix is <= 0 or not finite, and never raises for one.  Between `cond(I)` ~ 1e8
and singular neither is specified: both return whatever float64 leaves of the inverse, and which of them says NaN first is
erratic there (in the reference as well).
"""
import math

import numpy as np

__all__ = ["crlb", "crlb_grad", "crlb_split", "confint"]


# ------------------------------------------------------------------------------------------------ device branch
def _device_kind(J):
    """'jacobian' for a DeviceJacobian, 'other' for any other device handle, None for host data"""
    from . import functions
    if isinstance(J, functions.DeviceJacobian):
        return "jacobian"
    if isinstance(J, (functions.DeviceSignal, functions.ShardedDeviceSignal)):
        return "other"
    return None


def _device_weights(J, W, sigma2):
    """W as the device path takes it (a vector of nparam values or None); raises for what it does not take"""
    nparam = len(J.rows)
    if W is not None:
        W = np.asarray(W)
        if W.ndim != 1 or W.shape[0] != nparam or W.dtype.kind not in "fiub":
            raise NotImplementedError(f"W: on a DeviceJacobian a real vector of nparam = {nparam} weights or None, got shape "
                                      f"{W.shape} ({W.dtype}); download the Jacobian for weights that vary over the grid")
    if np.ndim(sigma2) != 0 or np.iscomplexobj(sigma2):
        raise NotImplementedError("sigma2: on a DeviceJacobian a real scalar; download the Jacobian for a noise map")
    return W


def _device_bounds(J, W, sigma2, log, split):
    from . import _lib
    nparam = len(J.rows)
    W = _device_weights(J, W, sigma2)
    buf = J._buf
    # (a handle whose buffer was freed hands over NULL: the library's EpgxError, as for a download)
    res = _lib.signal_crlb(buf.ctx, J.ptr if buf.ptr else None, J.record_stride, J.row_stride, J._nrow,
                           J.nrec, J.rows, 0, J.nvox, weights=W, sigma2=float(sigma2), split=split, log=log)
    return res.reshape(((nparam,) if split else ()) + J.grid)


# ------------------------------------------------------------------------------------------------ host branch
def _normal_matrix(A):
    """Re(A^H A) over the point axis of A [..., npoint, nparam]: real and symmetric, [..., nparam, nparam]"""
    return np.matmul(np.conj(A).swapaxes(-1, -2), A).real


def _fisher_inverse(J, sigma2):
    """(J [..., npoint, nparam] as an array, the inverse Fisher matrix of every voxel [..., nparam, nparam], the noise
    factor 1 / sigma2 per voxel [...]).  Voxels whose Fisher matrix has a condition number above 1e30 become NaN."""
    J = np.asarray(J)
    gram = _normal_matrix(J)
    noise = np.broadcast_to(np.reciprocal(np.asarray(sigma2, dtype=np.float64)), gram.shape)
    fisher = noise * gram
    singular = np.linalg.cond(fisher) > 1e30
    if np.any(singular):
        fisher[singular] = np.nan
    return J, np.linalg.inv(fisher), noise[..., 0, 0]


def _reject_handles(J):
    kind = _device_kind(J)
    if kind == "other":
        raise NotImplementedError(f"J: {type(J).__name__}; the device path takes the DeviceJacobian of a run on one GPU")
    return kind == "jacobian"


def crlb(J, H=None, *, W=None, sigma2=1, log=False):
    """Cramer-Rao lower bound as a cost: `sum_p W_p lb_pp` with `lb = (1 / sigma2 Re(J^H J))^-1`, per voxel.

    J: Jacobian `[..., npoint, nparam]` (NumPy), or a DeviceJacobian (its records are the points; see the module docstring).
    H: second derivatives `[..., npoint, nparam, nx]` of the signal with respect to nx design variables (host arrays only):
       the return value is then `(cost, grad)` with `grad [..., nx]`.
    W: weights of the parameters, broadcast against `[..., nparam]` (device: a vector of nparam values); sigma2: noise
       variance, a scalar or an array that broadcasts against `[..., nparam, nparam]` (device: a scalar); log: return log10
       of the cost (and the gradient of that).
    Returns `[...]` (device: float64 `grid`).  Singular voxels give NaN (module docstring)."""
    if _reject_handles(J):
        if H is not None:
            raise NotImplementedError("H: crlb takes second derivatives as host arrays only; stats.crlb_grad(J, H) computes cost and "
                                      "gradient from a DeviceJacobian and a DeviceHessian on the device (or download both with np.asarray)")
        return _device_bounds(J, W, sigma2, log, split=False)

    J, lb, noise = _fisher_inverse(J, sigma2)
    variances = np.diagonal(lb, axis1=-2, axis2=-1)
    weights = np.ones(J.shape[-1]) if W is None else np.asarray(W)
    cost = np.sum(weights * variances, axis=-1)
    if H is None:
        return np.log10(cost) if log else cost
    # cost = tr(D lb), D = diag(W), lb = F^-1:  d cost = -tr(D lb dF lb) = -sum_ab S_ab dF_ab  with  S = lb D lb (symmetric)
    # and dF_ab = noise * (conj(dJ_ka) J_kb + conj(J_ka) dJ_kb).real summed over the points k.  Both halves give the same
    # sum against the symmetric S, so  d cost / dx = -2 noise * sum_kb Re( conj(H_kbx) * (J S)_kb ).
    S = np.matmul(lb * weights[..., np.newaxis, :], lb)
    JS = np.matmul(J, S)
    grad = -2.0 * noise[..., np.newaxis] * np.sum((np.conj(np.asarray(H)) * JS[..., np.newaxis]).real, axis=(-3, -2))
    if log:      # d log10(c) = dc / (c ln 10)
        return np.log10(cost), grad / (cost[..., np.newaxis] * math.log(10.0))
    return cost, grad


MAX_DEVICE_PARAMS = 4      # CRLB_MAX_P of csrc/epgx_stats.h


def crlb_grad(J, H, *, W=None, sigma2=1, log=False):
    """The cost of `crlb` and its gradient with respect to nx design variables: `(cost, grad)`.

    On the device: J a DeviceJacobian and H a DeviceHessian of the same run parameters -- `Jacobian(params)` and
    `Hessian(params, design)` from two `simulate(..., out="device")` calls on one GPU, the same grid and records,
    `J.variables == H.variables1`.  Returns float64 `cost` of shape `grid` and `grad` of shape `grid + (nx,)`, nx =
    `len(H.variables2)`; the cost has the bits of `crlb(J, ...)`.  W a vector of nparam values or None, sigma2 a scalar, at most
    4 parameters, as for `crlb` on a DeviceJacobian.  A singular voxel has NaN in the cost and in its whole gradient.
    On host arrays (J `[..., npoint, nparam]`, H `[..., npoint, nparam, nx]`): exactly `crlb(J, H=H, ...)`."""
    from . import functions, _lib
    kinds = {}
    for name, arg, handle in (("J", J, functions.DeviceJacobian), ("H", H, functions.DeviceHessian)):
        if isinstance(arg, handle):
            kinds[name] = True
        elif isinstance(arg, (functions.DeviceSignal, functions.ShardedDeviceSignal, functions.DeviceJacobian, functions.DeviceHessian)):
            raise NotImplementedError(f"{name}: {type(arg).__name__}; the device path takes a {handle.__name__} of a run on one GPU")
        else:
            kinds[name] = False
    if not kinds["J"] and not kinds["H"]:
        return crlb(J, H=H, W=W, sigma2=sigma2, log=log)
    if not kinds["H"]:
        raise NotImplementedError("H: a host array next to a DeviceJacobian; download J (np.asarray, records to axis -2) and call "
                                  'crlb(J, H=H), or compute H with out="device" too')
    if not kinds["J"]:
        raise NotImplementedError("J: a host array next to a DeviceHessian; download H (np.asarray, records to axis -3) and call "
                                  'crlb(J, H=H), or compute J with out="device" too')
    if J._buf.ctx is not H._buf.ctx or J.device != H.device:
        raise ValueError(f"H: lives on device {H.device} in another context than J (device {J.device}); both must come from one GPU context")
    if J.grid != H.grid or J.nrec != H.nrec:
        raise ValueError(f"H: {H.nrec} records over the grid {H.grid}, J has {J.nrec} records over {J.grid}")
    if list(J.variables) != list(H.variables1):
        raise ValueError(f"H: variables1 = {H.variables1} must be the variables of J, {J.variables}, in this order")
    nparam = len(J.rows)
    if nparam > MAX_DEVICE_PARAMS:
        raise NotImplementedError(f"J: {nparam} parameters; the device path takes up to {MAX_DEVICE_PARAMS}, download J and H for more")
    W = _device_weights(J, W, sigma2)
    cost, grad = _lib.signal_crlb_grad(J._buf.ctx, J.ptr if J._buf.ptr else None, J.record_stride, J.row_stride, J._nrow, J.nrec, J.rows,
                                       0, J.nvox, H.ptr if H._buf.ptr else None, H._buf.nbytes // 16, H.offsets, H.record_strides,
                                       weights=W, sigma2=float(sigma2), log=log)
    return cost.reshape(J.grid), np.ascontiguousarray(grad.T).reshape(J.grid + (grad.shape[0],))


def crlb_split(J, W=None, sigma2=1, log=False):
    """Cramer-Rao lower bound of every parameter: `W_p lb_pp`, `[nparam, ...]` (device: float64 `[nparam, *grid]`); arguments
    as for `crlb`"""
    if _reject_handles(J):
        return _device_bounds(J, W, sigma2, log, split=True)
    _, lb, _ = _fisher_inverse(J, sigma2)
    variances = np.diagonal(lb, axis1=-2, axis2=-1)
    if W is not None:
        variances = variances * np.asarray(W)
    variances = np.moveaxis(variances, -1, 0)
    return np.log10(variances) if log else np.array(variances)


def confint(obs, pred, jac, hess=None, *, conflevel=0.95):
    """Delta-method confidence intervals of a least-squares fit (host arrays only).

    obs, pred `[..., nobs]`; jac `[..., nobs, nparam]`; hess `[..., nobs, nparam, nparam]` or None (then the Gauss-Newton
    normal matrix `Re(J^H J)` alone stands in for the Hessian of the cost).  Returns `(cints [..., nparam], cband [..., nobs])`:
    the half-widths of the intervals of the parameters and of the band around the prediction at `conflevel`."""
    if any(_device_kind(a) for a in (obs, pred, jac, hess)):
        raise NotImplementedError("confint is host-only: download the arrays first (np.asarray)")
    jac = np.asarray(jac)
    npoint, nparam = jac.shape[-2], jac.shape[-1]
    freedom = npoint - nparam
    misfit = np.asarray(obs) - np.asarray(pred)
    variance = np.sum(np.abs(misfit) ** 2, axis=-1) / freedom           # residual variance of the fit
    curvature = _normal_matrix(jac)
    if hess is not None:
        # second-order term as the reference defines it: the second derivatives summed over the points, times the summed
        # residual (indices of the second derivatives transposed)
        second = np.conj(np.asarray(hess)).sum(axis=-3).swapaxes(-1, -2) * misfit.sum(axis=-1)[..., np.newaxis, np.newaxis]
        curvature = second.real + curvature
    covariance = np.linalg.inv(curvature) * variance[..., np.newaxis, np.newaxis]
    tval = _t_interval(conflevel, freedom)
    param_var = np.diagonal(covariance, axis1=-2, axis2=-1)
    band_var = np.sum(np.matmul(np.conj(jac), covariance) * jac, axis=-1).real           # J cov J^H, its diagonal
    return tval * np.sqrt(param_var), tval * np.sqrt(band_var)


# ------------------------------------------------------------------------------------------------ Student t
def _betacf(a, b, x):
    """continued fraction of the incomplete beta function (modified Lentz), converges fast for x < (a + 1) / (a + b + 2)"""
    tiny = 1e-300
    c, d = 1.0, 1.0 - (a + b) * x / (a + 1.0)
    d = 1.0 / (d if abs(d) > tiny else tiny)
    h = d
    for m in range(1, 10000):
        for num in (m * (b - m) * x / ((a + 2 * m - 1) * (a + 2 * m)),
                    -(a + m) * (a + b + m) * x / ((a + 2 * m) * (a + 2 * m + 1))):
            d = 1.0 + num * d
            d = 1.0 / (d if abs(d) > tiny else tiny)
            c = 1.0 + num / c
            c = c if abs(c) > tiny else tiny
            h *= d * c
        if abs(d * c - 1.0) < 1e-16:
            return h
    raise ArithmeticError(f"incomplete beta function: no convergence at a={a}, b={b}, x={x}")


def _betainc(a, b, x):
    """regularised incomplete beta function I_x(a, b)"""
    if x <= 0.0:
        return 0.0
    if x >= 1.0:
        return 1.0
    front = math.exp(math.lgamma(a + b) - math.lgamma(a) - math.lgamma(b) + a * math.log(x) + b * math.log1p(-x))
    if x < (a + 1.0) / (a + b + 2.0):
        return front * _betacf(a, b, x) / a
    return 1.0 - front * _betacf(b, a, 1.0 - x) / b


def _t_tails(t, dof):
    """probability of |T| > t for Student's t with `dof` degrees of freedom, t >= 0"""
    return _betainc(0.5 * dof, 0.5, dof / (dof + t * t))


_T_INTERVAL = {}


def _t_interval(conflevel, dof):
    """t such that P(|T| <= t) = conflevel for Student's t with `dof` degrees of freedom (the upper end of
    scipy.stats.t.interval): bisection on the two-sided tail probability, which is the regularised incomplete beta function
    I_{dof / (dof + t^2)}(dof / 2, 1 / 2) -- no cancellation for conflevel near 1"""
    conflevel, dof = float(conflevel), float(dof)
    if not (0.0 < conflevel < 1.0) or not dof > 0.0:
        raise ValueError(f"confint: conflevel = {conflevel} must lie in (0, 1) and dof = {dof} be positive")
    key = (conflevel, dof)
    if key not in _T_INTERVAL:
        tail = 1.0 - conflevel
        lo, hi = 0.0, 1.0
        while _t_tails(hi, dof) > tail:
            lo, hi = hi, 2.0 * hi
        for _ in range(200):
            mid = 0.5 * (lo + hi)
            if mid == lo or mid == hi:
                break
            if _t_tails(mid, dof) > tail:
                lo = mid
            else:
                hi = mid
        _T_INTERVAL[key] = 0.5 * (lo + hi)
    return _T_INTERVAL[key]

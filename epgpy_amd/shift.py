"""Shift operator S (mirrors epgpy/shift.py:14-158, integer 1-D branch).

`S(k)` with a Python int k moves F_j -> F_{j+k}: the number of states grows by |k| up to
`max_nstate` (option on the state matrix, shift.py:86) or this operator's `nmax`; beyond
that the highest order is dropped (shift.py:98, :283-287).  On the device this is a DPP
wave shift (|k| = 1) or an LDS-staged permutation (|k| > 1) inside the fused kernel.
Integer vectors -- one for all voxels, or one per point of the leading grid axes -- take the host-planned
gather shift (kspace.py).  Float wavenumbers -- `S(1.5)`, the gradient `G(tau, gradient)`, the time accumulation `C(tau, R2)`,
or any shift of coordinates that already are float -- take the shift-merge (kmerge.py): rows that fall into one cell of the
grid `kgrid` merge, on the device, between two reductions of the resident state.  Such a shift is a barrier of the
operator-by-operator path.  A float wavenumber that varies along a grid axis (shift-prune: `S([[1.5], [0.5]])`, `G` with an
array of gradients, `C` with an array `R2`) gives every voxel its own coordinate set: with the option `voxel_coords=True` of
the state matrix / of simulate() the device sorts, merges, trims and prunes per voxel (kmerge.shift_prune); without it the
shift raises as before.
"""
import numpy as np

from . import common, operator, utils, _lib


def _is_float(ks):
    from . import kmerge
    return kmerge.is_float(ks)


class S(operator.Operator):
    def __init__(self, k, *, nmax=None, kgrid=None, prune=1e-8, name=None, duration=None):
        if np.allclose(k, 0):
            raise TypeError("Cannot have k == 0")
        if isinstance(k, (int, np.integer)) and not isinstance(k, bool):
            k = int(k)
        else:
            k = np.atleast_2d(k)
            if k.shape[-1] not in [1, 2, 3, 4]:
                raise ValueError("k.shape[-1] must belong to [1, 2, 3, 4]")
        self.k, self.nmax, self.prune, self.kgrid = k, nmax, prune, kgrid
        if not name:
            name = common.repr_operator("S", ["k"], [k], ["" if isinstance(k, int) else ".2f"])
        super().__init__(name=name, duration=duration)

    @property
    def nshift(self):
        if common.isscalar(self.k):
            return abs(self.k)
        return np.round(np.max(abs(self.k))).astype(int)

    @property
    def shape(self):
        return (1,) if common.isscalar(self.k) else self.k.shape[:-1]

    @property
    def kdim(self):
        return 1 if common.isscalar(self.k) else self.k.shape[-1]

    def __call__(self, sm, *, inplace=False):
        """S has no parameters but is a DiffOperator in the reference (shift.py:14): derivative states
        attached to `sm` are shifted with it"""
        order1, order2 = getattr(sm, "order1", None), getattr(sm, "order2", None)
        if (order1 or order2) and (self._float_k() or _is_float(sm._kspace)):
            raise NotImplementedError("derivative states (order1 / order2, Jacobian / Hessian) through a float shift (shift-merge)")
        sm = super().__call__(sm, inplace=inplace)
        if order1 or order2:
            from . import diff
            sm.order1 = diff.propagate_plain(self, sm, order1 or {}, inplace)
            sm.order2 = diff.propagate_plain(self, sm, order2 or {}, inplace)
        return sm

    def _float_k(self):
        """True for a float wavenumber: the shift is a shift-merge whatever the coordinates are (shift.py:213-254)"""
        return not isinstance(self.k, int) and not np.issubdtype(self.k.dtype, np.integer)

    def _encode(self, enc):
        # shift.py:86: the state-matrix option wins over the operator's own nmax
        nmax = enc.options.get("max_nstate") or self.nmax or None
        if self._float_k() or _is_float(enc.kspace):
            if (enc.options.get("kgrid") or self.kgrid) is None:
                raise AttributeError("kgrid not set")        # the reference's own error (shift.py:131-132)
            if np.sum(np.shape(self.k)[:-1]) > 1:
                raise NotImplementedError("a float wavenumber that varies along a grid axis (shift-prune, shift.py:247-249, "
                                          ":478-542): the coordinate sets would differ per voxel; the option voxel_coords=True "
                                          "runs it per voxel, operator by operator (simulate / op(sm)), not in a compiled plan")
            raise NotImplementedError("a float shift (shift-merge, shift.py:367-449) cannot be compiled into a plan: it runs "
                                      "operator by operator (simulate(mode='stepwise') or op(sm))")
        if isinstance(self.k, int):
            enc.add_shift(self.k, nmax)                      # 'shift-1d' (or [k,0,..] once coords exist)
            return
        # 'shift-nd', shift.py:103-118; a vectorised k (one vector per point of the leading grid axes) keeps ONE row
        # structure for all voxels, only the coordinates of the rows then differ per voxel (kspace.py)
        enc.add_gather_shift(self.k[0] if self.k.shape[:-1] == (1,) else self.k, nmax)


class G(S):
    """gradient operator (shift.py:163-185): the shift by the wavenumber (rad/m) that a gradient `gradient` (mT/m, a scalar or
    up to three components) accumulates in `tau` ms"""

    def __init__(self, tau, gradient, *, duration=None, **kwargs):
        tau, gradient = common.map_arrays([tau, gradient])
        if np.any(np.asarray(tau) < 0):
            raise ValueError("Cannot have negative time")
        if not common.isscalar(gradient) and common.get_shape(gradient)[-1] > 3:
            raise ValueError("Only 3d gradients are allowed")
        k = utils.get_wavenumber(tau, gradient)
        self.tau, self.gradient = tau, gradient
        super().__init__(k, duration=tau if duration is True else duration, **kwargs)


class C(S):
    """time accumulation for temporal dephasing (T2', T2*; shift.py:188-208): `tau * R2` is added to the fourth coordinate,
    which `F0` weighs by exp(-|t|)"""

    def __init__(self, tau, R2=1, *, duration=None, **kwargs):
        tau, R2 = common.map_arrays([tau, R2])
        if np.any(np.asarray(tau) < 0):
            raise ValueError("Cannot have negative time")
        evol = tau * R2
        k = np.stack([0 * evol] * 3 + [evol], axis=-1)       # time on the fourth dimension
        self.tau, self.R2 = tau, R2
        super().__init__(k, duration=tau if duration is True else duration, **kwargs)

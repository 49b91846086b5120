"""Probe operators (mirrors epgpy/probe.py:7-165, :223).

`ADC` (= `Adc("F0")`) is the hot-path read-out: inside the fused kernel lane 0 of each
wavefront stores F_0 (or Z_0) of its voxel into the signal buffer, so nothing is copied
per ADC.  Weights / reduction / phase compensation (probe.py:141-165) are applied on the
host to the downloaded signal.  General probes (eval'd expressions, callables, "F", "Z",
...) need the whole state on the host: `simulate` then falls back to segment-wise execution
and evaluates them on a downloaded StateMatrix view.

`DFT` / `Imaging` (probe.py:168-219) read the state out in space.  The sum over phase states runs on the device-resident state
(csrc/epgx_dft.hip through epgx_state_dft), weights and sums over axes of the image on the device as well
(epgx_signal_reduce): only the record the caller asked for crosses PCIe.
"""
import numpy as np

from . import common, operator, utils, _lib

SM_LOCALS = ["nstate", "ndim", "kdim", "states", "coords", "F", "F0", "F0t", "Z", "Z0", "k", "t", "t0"]
DEVICE_KINDS = {"F0": 0, "Z0": 1}


class _LazyAttrs(dict):
    """names resolved from a StateMatrix only when the expression touches them"""

    def __init__(self, sm, extra):
        super().__init__(extra)
        self._sm = sm

    def __missing__(self, key):
        if key in SM_LOCALS:
            return getattr(self._sm, key)
        raise KeyError(key)


class Probe(operator.EmptyOperator):
    """records data; does not modify the state (probe.py:7-79)"""

    SM_LOCALS = SM_LOCALS

    def __init__(self, obj, *args, post=None, **kwargs):
        if isinstance(obj, str):
            self._expr = obj
            self._acquire = self._acquire_expr
        elif callable(obj):
            self._callable = obj
            self._acquire = self._acquire_callable
        else:
            raise TypeError(f"Invalid probe: {obj}")
        self._args, self._kwargs = args, kwargs
        self._post = post
        self._repr = f"'{obj}'"
        super().__init__()

    def _device_kind(self):
        """0 / 1 if the kernel can record this probe itself (F0 / Z0), else None"""
        expr = getattr(self, "_expr", None)
        if expr is not None and expr.strip() in DEVICE_KINDS and not self._kwargs:
            return DEVICE_KINDS[expr.strip()]
        return None

    def _finish(self, raw):
        """turn the raw device record into what `_acquire` would have returned"""
        return raw

    def _is_plain(self):
        """True if neither `_finish` nor `post` changes a device record"""
        return (type(self)._finish is Probe._finish and type(self).post is Probe.post
                and not getattr(self, "_post", None) and not hasattr(self, "_assemble"))

    def _acquire_expr(self, sm):
        return eval(self._expr, vars(np), _LazyAttrs(sm, self._kwargs))  # noqa: S307 (reference semantics)

    def _acquire_callable(self, sm):
        return self._callable(sm, *self._args, **self._kwargs)

    def acquire(self, sm, post=None):
        post = post if post else self.post
        return post(common.asnumpy(self._acquire(sm), copy=True))

    def post(self, obj):
        if not getattr(self, "_post", None):
            return obj
        return self._post(obj)

    def __call__(self, sm, **kwargs):
        return sm

    def __repr__(self):
        return self.name or f"Probe({self._repr})"


def _trailing(arr, ndim):
    """`arr` with size-1 axes appended up to `ndim` axes (parameters align with the LEADING grid axes)"""
    arr = np.asarray(arr)
    return arr.reshape(arr.shape + (1,) * (ndim - arr.ndim)) if (arr.size > 1 and arr.ndim < ndim) else arr


def _reduction_axes(reduce, weights):
    """normalised `reduce` argument of Adc: None / False (keep everything), True (sum everything) or a tuple of axes.
    With weights and no explicit `reduce`, the sum runs over the axes of the weights (probe.py:110-131)."""
    if reduce is not None and reduce is not True and reduce:
        axes = (reduce,) if isinstance(reduce, int) else tuple(reduce)
        if any(not isinstance(ax, int) for ax in axes):
            raise ValueError(f"Expected (tuple of) int, got: {axes}")
        reduce = axes
    if weights is not None:
        span = max(weights.ndim, 1)
        if reduce is None:
            reduce = tuple(range(span))
        elif reduce is not True and reduce and not set(reduce) <= set(range(span)):
            raise ValueError(f"Invalid reduce dimension(s): {reduce}")
    return reduce


class Adc(Probe):
    """probe of one StateMatrix attribute, optionally weighted, summed over grid axes and phase-compensated
    (probe.py:82-165).  Three independent post-processing steps, applied in this order:
        record * weights  ->  sum over `reduce`  ->  * exp(i phase)          (phase in degrees, applied by `post`)
    F0 / Z0 records come straight out of the kernel; weights + reduce then run on the device (epgx_signal_reduce)."""

    def __init__(self, attr="F0", *, phase=None, reduce=None, weights=None, name="ADC"):
        if attr not in self.SM_LOCALS:
            raise ValueError(f"Invalid StateMatrix attribute: {attr}")
        self.attr = attr
        self.weights = None if weights is None else np.asarray(weights)
        self.reduce = _reduction_axes(reduce, self.weights)
        self.phase = None if phase is None else np.asarray(phase)
        if self.phase is not None:
            self.phasor = np.exp(1j * self.phase / 180 * np.pi)
        self._repr = attr if phase is None else f"'{attr}', {common.repr_value(phase, '.1f')}"
        operator.Operator.__init__(self, name=name)

    def _device_kind(self):
        return DEVICE_KINDS.get(self.attr)

    def _is_plain(self):
        return self.weights is None and (self.reduce is None or self.reduce is False) and self.phase is None

    def _device_reduction(self, grid):
        """(reduce mask over the grid axes, weights or None) if the device can do `_finish`
        (epgx_signal_reduce), else None: then the record is downloaded and finished on the host"""
        if self.reduce is None or self.reduce is False or self.reduce == ():
            return None
        ndim = len(grid)
        if self.reduce is True:
            mask = [1] * ndim
        else:
            axes = (self.reduce,) if isinstance(self.reduce, int) else self.reduce   # reduce=0 stays an int (probe.py:113-118)
            axes = [ax + ndim if ax < 0 else ax for ax in axes]
            if any(ax < 0 or ax >= ndim for ax in axes) or len(set(axes)) != len(axes):
                return None          # let NumPy raise its own error on the host path
            mask = [1 if d in axes else 0 for d in range(ndim)]
        weights = self.weights
        if weights is not None:
            if weights.ndim > ndim or weights.dtype.kind not in "fciub" or any(
                    w not in (1, g) for w, g in zip(weights.shape, grid)):
                return None
        return mask, weights

    def _finish(self, arr):
        if self.weights is not None:
            arr = arr * _trailing(self.weights, arr.ndim)
        if self.reduce is None or self.reduce is False:
            return arr
        return arr.sum() if self.reduce is True else arr.sum(axis=self.reduce)

    def _acquire(self, sm):
        return self._finish(getattr(sm, self.attr))

    def _post(self, obj):
        arr = np.asarray(obj)
        return arr if self.phase is None else arr * _trailing(self.phasor, arr.ndim)


# ------------------------------------------------------------------------------------------------ spatial read-out
READOUT_SLAB_BYTES = 8 << 30     # device temporaries of one slab of voxels (image + coefficient table) stay below this
READOUT_MAX_VOXELS = 65535 * 256  # voxels of one epgx_state_dft call


def readout_tables(kspace, nstate, kvalue, ncol, voxel_shape="box", voxel_size=1, tol=1e-8):
    """what epgx_state_dft needs to know about the STORED orders j = 0 .. nstate of a state matrix, per voxel class:
    (k [L, nstate + 1, ncol] wavenumbers in rad/m that enter the phase, w [L, nstate + 1] voxel factors, lead).
    `kspace`: the planner's coordinate set (kspace.KSpace; its `lead` axes are a leading part of the grid, L = prod(lead)
    classes) or None for the 1-D orders 0 .. nstate.  Wavenumbers as `StateMatrix.k`: coordinate x kvalue, at most three
    columns.  The factor runs over ALL columns; an order is dropped (w = 0 in every class) unless its factor exceeds `tol`
    in some class -- the `kmask` rule of utils.imaging, which row k and row -k pass or fail together (sinc is even)."""
    if kspace is None:
        half, lead = np.arange(nstate + 1, dtype=np.int64).reshape(1, nstate + 1, 1), ()
    else:
        half, lead = np.moveaxis(kspace.points[kspace.centre:], 0, 1), kspace.lead      # [L, nrow, kdim]
    if half.shape[1] != nstate + 1:
        raise ValueError(f"coordinates of {half.shape[1]} stored orders for a state matrix with nstate={nstate}")
    kv = kvalue if common.isscalar(kvalue) else np.asarray(kvalue, dtype=np.float64)[: half.shape[-1]]
    k = (half * kv)[..., :3].astype(np.float64)
    if ncol > k.shape[-1]:
        raise ValueError(f"positions with {ncol} columns for wavenumbers with {k.shape[-1]}")
    w = utils.voxel_factor(k, voxel_shape, voxel_size)
    if voxel_shape == "box":
        w = np.where(np.any(np.abs(w) > tol, axis=0), w, 0.0)
    else:
        w = np.ones(k.shape[:2])
    return np.ascontiguousarray(k[..., :ncol]), np.ascontiguousarray(w), lead


def class_ranges(shape, lead):
    """[(first voxel, one past the last, class)] of a grid `shape` whose coordinate classes live on the axes `lead` (a leading
    part of the grid, append rule): contiguous voxel ranges, neighbours of one class merged"""
    nl = len(lead)
    outer = tuple(shape[:nl])
    chunk = int(np.prod(shape[nl:], dtype=np.int64))
    nclass = int(np.prod(lead, dtype=np.int64))
    owner = np.broadcast_to(np.arange(nclass).reshape(tuple(lead)), outer).reshape(-1) if nl else np.zeros(1, np.int64)
    ranges = []
    for i, cls in enumerate(owner):
        if ranges and ranges[-1][2] == cls:
            ranges[-1][1] = (i + 1) * chunk
        else:
            ranges.append([i * chunk, (i + 1) * chunk, int(cls)])
    return [tuple(r) for r in ranges]


def _image_reduction(reduce, weights, shape):
    """(mask over the axes of the image, weights aligned with them or None) if epgx_signal_reduce can finish the image, else
    None.  `reduce` as utils.imaging: True / None sum everything, an int / tuple those axes; weights follow NumPy broadcasting"""
    ndim = len(shape)
    if reduce is False or ndim > _lib.MAX_DIMS:
        return None
    if reduce is True or reduce is None:
        mask = [1] * ndim
    else:
        try:
            axes = [int(ax) for ax in ((reduce,) if np.ndim(reduce) == 0 else reduce)]
        except (TypeError, ValueError):
            return None
        axes = [ax + ndim if ax < 0 else ax for ax in axes]
        if not axes or any(ax < 0 or ax >= ndim for ax in axes) or len(set(axes)) != len(axes):
            return None                  # (nothing to sum, or NumPy's own error on the host)
        mask = [1 if ax in axes else 0 for ax in range(ndim)]
    if weights is not None:
        weights = weights.reshape((1,) * (ndim - weights.ndim) + weights.shape)
    return mask, weights


def _weights_fit(weights, shape):
    """True if `image *= weights` is defined for an image of `shape` (real / complex weights that broadcast to it)"""
    if weights.dtype.kind not in "fciub" or weights.ndim > len(shape):
        return False
    return all(w in (1, g) for w, g in zip(weights.shape[::-1], shape[::-1]))


def read_out(sm, positions, *, phase=None, weights=None, modulation=None, voxel_shape="box", voxel_size=1, expand=True,
             reduce=True, tol=1e-8):
    """utils.imaging of the state matrix `sm` at `positions`.  On the device when the request is one epgx_state_dft covers:
    `expand`, a "point" or "box" voxel, no or a scalar `phase`, at most three position columns (and no more than the
    wavenumbers have), weights that broadcast to the image; anything else goes through utils.imaging on the downloaded
    `sm.F` / `sm.k`.  A state matrix with a time coordinate (operator C: kdim = 4) takes that host path as well, with
    `acctime=sm.t` and `modulation` (decay rate and frequency of the accumulated time, utils.imaging); while kdim < 4
    `modulation` has no effect, as in the reference.  State matrices live at the library's capacities (up to 1024 orders),
    all of which the kernel covers."""
    from . import kmerge
    if isinstance(sm._kspace, kmerge.VoxelKSpace):
        raise NotImplementedError("DFT / Imaging on per-voxel coordinates (shift-prune, voxel_coords): the spatial read-out takes "
                                  "coordinates shared by all voxels")
    pos = np.asarray(positions)
    pos = pos if pos.ndim > 1 else pos[..., np.newaxis]
    wts = None if weights is None else np.asarray(weights)
    image_shape = sm.shape + pos.shape[:-1]
    nk = 1 if sm._kspace is None else min(sm._kspace.kdim, 3)
    on_device = (expand and voxel_shape in ("point", "box") and (phase is None or np.ndim(phase) == 0)
                 and pos.dtype.kind in "fiu" and 1 <= pos.shape[-1] <= nk and pos.size > 0
                 and (wts is None or _weights_fit(wts, image_shape))
                 and (sm._kspace is None or sm._kspace.nstate == sm.nstate)
                 and sm.nstate + 1 <= sm._state.K)      # (a state matrix truncated at its capacity: the host view pads it)
    if sm.kdim == 4:
        return utils.imaging(positions, sm.F, sm.k[..., :3], sm.t, phase=phase, weights=weights, modulation=modulation,
                             voxel_shape=voxel_shape, voxel_size=voxel_size, expand=expand, reduce=reduce, tol=tol)
    if not on_device:
        return utils.imaging(positions, sm.F, sm.k[..., :3], phase=phase, weights=weights, modulation=modulation,
                             voxel_shape=voxel_shape, voxel_size=voxel_size, expand=expand, reduce=reduce, tol=tol)

    k_tab, w_tab, lead = readout_tables(sm._kspace, sm.nstate, sm.kvalue, pos.shape[-1], voxel_shape, voxel_size, tol)
    phasor = 1.0 if phase is None else np.exp(1j * float(phase) * np.pi / 180)
    flat = np.ascontiguousarray(pos.reshape(-1, pos.shape[-1]), dtype=np.float64)
    nvox, npos, ctx = sm.size, len(flat), sm._ctx
    ranges = class_ranges(sm.shape, lead)
    plan = _image_reduction(reduce, wts, image_shape)
    slab = int(max(1, min(nvox, READOUT_MAX_VOXELS, READOUT_SLAB_BYTES // (16 * npos + 32 * (sm.nstate + 1)))))
    image = None if plan is not None else np.empty((nvox, npos), dtype=np.complex128)
    total = None
    for v0 in range(0, nvox, slab):
        n = min(slab, nvox - v0)
        buf = _lib.DeviceBuffer(ctx, 16 * n * npos)
        for first, last, cls in ranges:            # one launch per coordinate class (and slab)
            first, last = max(first, v0), min(last, v0 + n)
            if first < last:
                _lib.state_dft(ctx, sm._state, first, last - first, k_tab[cls], w_tab[cls], flat, phasor,
                               buf.ptr.value + 16 * (first - v0) * npos)
        if plan is not None:                        # the image is ONE record over the grid (*grid, *positions)
            part = _lib.signal_reduce(ctx, buf.ptr.value, n * npos, 0, 1, 1, image_shape, plan[0], plan[1],
                                      vox0=v0 * npos, nvox=n * npos)[0]
            total = part if total is None else total + part
        else:
            buf.download(np.complex128, (n, npos), out=image[v0:v0 + n])
        buf.free()
    if plan is not None:
        return total[()] if total.ndim == 0 else total
    image = image.reshape(image_shape)
    if wts is not None:
        image *= wts
    if reduce is False:
        return image
    return image.sum() if reduce is True else image.sum(axis=reduce)


class DFT(Probe):
    """discrete Fourier transform of the F states at `coords` (m; [*P, d] or 1-D), nothing summed: [*grid, *P] per
    acquisition (probe.py:168-181).  Without `coords` the positions are `sm.system["coords"]` (operator.System)."""

    def __init__(self, coords=None, *, name=None):
        self.coords = None if coords is None else np.asarray(coords)
        self._repr = "DFT"
        operator.Operator.__init__(self, name=name or "DFT")

    def _device_kind(self):
        return None

    def _acquire(self, sm):
        coords = self.coords if self.coords is not None else sm.system["coords"]
        return read_out(sm, coords, voxel_shape="point", reduce=False)


class Imaging(Probe):
    """imaging read-out: the F states summed at `coords` with a voxel shape, weights, a phase and a reduction -- the
    keywords of utils.imaging (probe.py:184-219).  Positions, `weights` and `modulation` come from the constructor, else
    from `sm.system` (operator.System).

    One deliberate difference from the reference: there `weights` / `modulation` given to the constructor are popped from
    the options at the first acquisition (probe.py:204-209), so an object that is acquired again has lost them.  Here they
    apply at EVERY acquisition."""

    def __init__(self, coords=None, *, name=None, **opts):
        self.coords = None if coords is None else np.asarray(coords)
        self._repr = "Imaging"
        self.opts = opts
        operator.Operator.__init__(self, name=name or "Imaging")

    def _device_kind(self):
        return None

    def _acquire(self, sm):
        opts = dict(self.opts)
        coords = self.coords if self.coords is not None else sm.system.get("coords", broadcast=False)
        for key in ("modulation", "weights"):
            if opts.get(key) is None:
                opts[key] = sm.system.get(key, broadcast=False)
        return read_out(sm, coords, **opts)


ADC = Adc(attr="F0", name="ADC")

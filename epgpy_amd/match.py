"""Dictionary matching on device handles: the consumer of a dictionary that `simulate(..., out="device")` leaves in HBM.

    from epgpy_amd import match
    dic = match.Dictionary(handle)          # computes and keeps n_a on the device
    res = match.match(dic, signals)         # .index, .scale, .score, .unravel()

With dictionary `D[t, a]` (records t, atoms a = the flattened grid) and measured signals `S[t, m]`, all complex128,

    n_a    = sum_t |D[t,a]|^2
    c[a,m] = sum_t conj(D[t,a]) S[t,m]            q[a,m] = |c[a,m]|^2 / n_a
    index[m] = argmax_a q[a,m]   over the atoms with a finite n_a > 0, the LOWEST a among equal q
    scale[m] = c[index,m] / n_index               the complex proton density:  S[:, m] ~ scale D[:, index]
    score[m] = sqrt(q[index,m] / sum_t |S[t,m]|^2)     in [0, 1]; 0 where the signal is identically zero

`norms_kernel`, `match_kernel` and `match_merge_kernel` (csrc/epgx_match.hip through `epgx_signal_norms` / `epgx_signal_match`)
read the dictionary where it lies; the correlation matrix [natoms, nmeas] is never stored and 32 bytes per measured voxel come
back over PCIe.  Where no atom is valid (all-zero atoms, atoms holding NaN) or the best q is not finite the voxel gets index -1,
scale 0, score 0.  A voxel's result does not depend on the other voxels of the call or on how the device splits the atoms.

Dictionaries: a `DeviceSignal` over the whole grid on one GPU (any probe of its buffer), a `DeviceJacobian` (its probed-state
row), or a NumPy array `[nrec, *grid]` (uploaded once).  Signals: a NumPy array `[nrec, *shape]` (real or complex; uploaded as
complex128) or a whole `DeviceSignal` on the same device.  Dictionaries of a run over several GPUs raise `NotImplementedError`.
"""
import numpy as np

__all__ = ["Dictionary", "MatchResult", "match"]


def _signal_handle(arg, name):
    """the DeviceSignal view of a device handle (None for host data); raises for handles the device path does not take"""
    from . import functions
    if isinstance(arg, functions.DeviceJacobian):
        # the probed-state row of every record: row 0 of the probe's block
        return functions.DeviceSignal(arg._buf, arg.nrec * arg._nprobe * arg._nrow, arg.grid, arg._j * arg._nrow, arg._nprobe * arg._nrow)
    if isinstance(arg, functions.ShardedDeviceSignal):
        raise NotImplementedError(f"{name}: a ShardedDeviceSignal (a run over several GPUs); match takes handles of one GPU -- "
                                  "download it (np.asarray) or simulate the dictionary on one device")
    if isinstance(arg, functions.DeviceHessian):
        raise NotImplementedError(f"{name}: a DeviceHessian holds no signal records; pass the DeviceSignal or DeviceJacobian of the run")
    if isinstance(arg, functions.DeviceSignal):
        if not arg.whole:
            raise NotImplementedError(f"{name}: a voxel slab [{arg.vox0}, {arg.vox0 + arg.count}) of the grid (a run over several GPUs); "
                                      "match takes handles that cover the whole grid on one GPU")
        return arg
    return None


class _Records:
    """complex128 records [nrec][ncol] on one device: a view of a DeviceSignal, or a host array uploaded into a buffer of its own"""

    def __init__(self, arg, name):
        handle = _signal_handle(arg, name)
        if handle is not None:
            self.keep, self.ctx = handle, handle._buf.ctx
            self.nrec, self.shape, self.ncol = handle.shape[0], tuple(handle.grid), handle.nvox
            self.row_stride = handle.row_stride
            self.device = handle.device
            return
        arr = np.asarray(arg)
        if arr.ndim < 1 or arr.dtype.kind not in "fciub":
            raise ValueError(f"{name}: an array [nrec, ...] of real or complex numbers, got shape {arr.shape} ({arr.dtype})")
        self.nrec, self.shape = arr.shape[0], tuple(arr.shape[1:])
        self.ncol = int(np.prod(self.shape, dtype=np.int64))
        self.row_stride = self.ncol
        self._host = np.ascontiguousarray(arr, dtype=np.complex128).reshape(self.nrec, self.ncol)
        self.keep, self.ctx, self.device = None, None, None

    def upload(self, ctx):
        """host records into a buffer of `ctx` (no-op for a handle)"""
        from . import _lib
        if self.keep is None:
            self.ctx, self.device = ctx, ctx.device
            self.keep = _lib.DeviceBuffer(ctx, max(self._host.nbytes, 16))
            if self._host.nbytes:
                self.keep.upload(self._host)
            del self._host

    @property
    def ptr(self):
        """address of record 0 (None when the buffer behind a handle was freed: the library's EpgxError)"""
        from . import _lib
        if isinstance(self.keep, _lib.DeviceBuffer):
            return self.keep.ptr.value if self.keep.ptr else None
        return self.keep.ptr if self.keep._buf.ptr else None


class Dictionary:
    """a dictionary on the device with its norms `n_a` (computed once, kept in HBM).

    handle: DeviceSignal over the whole grid, DeviceJacobian (its probed-state row), or a NumPy array `[nrec, *grid]`.
    `.grid`, `.natoms`, `.nrec`; `.norms` downloads `n_a` as float64 `grid`."""

    def __init__(self, handle, device=None):
        from . import _lib
        rec = handle if isinstance(handle, _Records) else _Records(handle, "dictionary")
        if len(rec.shape) == 0 and rec.keep is None:
            raise ValueError(f"dictionary: an array [nrec, *grid] with at least one grid axis, got shape ({rec.nrec},)")
        if rec.nrec < 1 or rec.ncol < 1:
            raise ValueError(f"dictionary: {rec.nrec} records of {rec.ncol} atoms; both must be at least 1")
        if rec.keep is None:
            rec.upload(_lib.get_context(device))
        self._rec = rec
        self.grid, self.natoms, self.nrec, self.device = rec.shape, rec.ncol, rec.nrec, rec.device
        self._norms = _lib.signal_norms(rec.ctx, rec.ptr, rec.row_stride, rec.nrec, rec.ncol)

    @property
    def norms(self):
        return self._norms.download(np.float64, (self.natoms,)).reshape(self.grid)


class MatchResult:
    """`index` int64 (flat index into the dictionary grid, -1: no valid atom), `scale` complex128, `score` float64, all of the
    shape of the measured voxels; `grid` the dictionary's grid"""

    def __init__(self, index, scale, score, grid):
        self.index, self.scale, self.score, self.grid = index, scale, score, tuple(grid)

    def unravel(self):
        """tuple of index arrays, one per grid axis (np.unravel_index); -1 stays -1 on every axis"""
        none = self.index < 0
        axes = np.unravel_index(np.where(none, 0, self.index), self.grid)
        return tuple(np.where(none, -1, ax) for ax in axes)


def match(dictionary, signals, *, nsplit=0):
    """best atom, complex scale and score of every measured voxel (module docstring).

    dictionary: a `Dictionary`, or anything `Dictionary` takes (its norms are then computed for this call).
    signals: NumPy array `[nrec, *shape]`, real or complex, or a whole DeviceSignal on the dictionary's device.
    nsplit: ranges the device cuts the atoms into (0: chosen by the library; the result does not depend on it).
    Returns a `MatchResult` whose arrays have the shape `signals.shape[1:]`."""
    from . import _lib
    sig = _Records(signals, "signals")
    if not isinstance(dictionary, Dictionary):
        # (checked before the dictionary touches the device)
        probe = _Records(dictionary, "dictionary")
        if probe.nrec != sig.nrec:
            raise ValueError(f"signals: {sig.nrec} records, the dictionary has {probe.nrec}")
        if sig.device is not None and probe.device is not None and sig.device != probe.device:
            raise ValueError(f"signals: on device {sig.device}, the dictionary on device {probe.device}; both must be on one GPU")
        dictionary = Dictionary(probe, device=sig.device)
    if dictionary.nrec != sig.nrec:
        raise ValueError(f"signals: {sig.nrec} records, the dictionary has {dictionary.nrec}")
    rec = dictionary._rec
    if sig.device is not None and (sig.device != rec.device or sig.ctx is not rec.ctx):
        raise ValueError(f"signals: on device {sig.device}, the dictionary on device {rec.device}; both must be on one GPU (and context)")
    sig.upload(rec.ctx)
    index, scale, score = _lib.signal_match(rec.ctx, rec.ptr, rec.row_stride, dictionary._norms.ptr.value if dictionary._norms.ptr else None,
                                            dictionary.natoms, sig.ptr, sig.row_stride, sig.nrec, sig.ncol, nsplit=nsplit)
    if isinstance(sig.keep, _lib.DeviceBuffer):
        sig.keep.free()        # (stream-ordered: the block is recycled behind the kernels that read it)
    return MatchResult(index.reshape(sig.shape), scale.reshape(sig.shape), score.reshape(sig.shape), dictionary.grid)

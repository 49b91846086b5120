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

SVD compression (`compress`, csrc/epgx_compress.hip through `epgx_signal_gram` / `epgx_signal_project`): matching is for short
fingerprints, and a long dictionary is made short without leaving HBM,

    basis = match.compress(dic, rank=8)        # or energy=0.9999
    res = match.match(basis.dictionary, signals)

    G[s,t]  = sum over valid a of D[s,a] conj(D[t,a])      on the device, [nrec, nrec] comes down
    G       = U diag(lambda) U^H                            on the host (numpy.linalg.eigh), lambda descending
    Dc[r,a] = sum_t conj(U[t,r]) D[t,a],  r < rank          on the device: the compressed dictionary [rank, *grid], in HBM
    Sc[r,m] = sum_t conj(U[t,r]) S[t,m]                     measured signals, projected the same way before matching

The Gram route resolves singular values down to about sqrt(u) sigma_0 only (u = 2^-53): `compress` refuses a rank that reaches
eigenvalues lambda_r <= nrec 2^-52 lambda_0.  That is far below what compression keeps (1e-4 .. 1e-6 of the energy).

Single precision (csrc/epgx_match32.hip through `epgx_signal_narrow` / `epgx_signal_norms_c64` / `epgx_signal_match_c64`):
`Dictionary(handle, dtype=np.complex64)`, `dictionary.astype(np.complex64)` or `compress(..., dtype=np.complex64)` give a
dictionary of 8 bytes per element.  It is DEFINED as the complex128 one rounded once (`astype(np.complex64)`, on the device for
a handle), and matching against it as the formulas above on the rounded dictionary and the rounded signals: n_a summed in
float64, c[a,m] in float32 on the fp32 MFMA, q, the comparison, scale and score in float64 from that c.  Results keep their
types.  The rate of the correlation doubles and every byte of dictionary and signals halves; c carries the error of a float32
inner product, about nrec 2^-22 sum_t |D||S| at most.

Dictionaries: a `DeviceSignal` over the whole grid on one GPU (any probe of its buffer), a `DeviceJacobian` (its probed-state
row), or a NumPy array `[nrec, *grid]` (uploaded once).  Signals: a NumPy array `[nrec, *shape]` (real or complex; uploaded as
complex128) or a whole `DeviceSignal` on the same device.  Dictionaries of a run over several GPUs raise `NotImplementedError`.

Off the grid (`refine`, csrc/epgx_refine.hip through `epgx_signal_refine`): a match ends at a grid point; one variable-projection
Gauss-Newton step at the matched atom, from the derivative rows of a `DeviceJacobian` that lie in HBM next to the dictionary,
moves it between the grid points,

    res = match.match(jac, signals)            # jac = simulate(..., probe=epg.Jacobian([...]), out="device")
    ref = match.refine(jac, signals, res)      # .delta, .scale, .score, .estimate([T1, T2])

For measured voxel `m` with atom `a = index[m]`: `d_t = D[t,a]`, `j_pt = J_p[t,a]` for `p < P`, `s_t = S[t,m]`, all complex128;
`P` = 1 ... 4 chosen columns of the Jacobian.  Accumulated over the records:

    n = sum |d|^2 (real)    E = sum |s|^2 (real)    c = sum conj(d) s    b_p = sum conj(j_p) s    h_p = sum conj(d) j_p
    M_pq = sum conj(j_p) j_q   (Hermitian, M_pp real; only Re M_pq enters below)

From those, per voxel and in float64:

    rho   = c / n                                       (match's scale, recomputed here from the same records)
    N_pq  = |rho|^2 Re(M_pq - conj(h_p) h_q / n)         Gauss-Newton matrix of  min over real delta of ||s - rho (d + J delta)||^2,
    y_p   = Re(conj(rho) (b_p - rho conj(h_p)))         rho projected out (Kaufman's variable projection)
    Nhat_pq = N_pq / (|rho|^2 sqrt(M_pp M_qq))           equilibrated by the UNPROJECTED column norms: pivots in [0, 1]
    delta = solution of N delta = y by Cholesky of Nhat
    delta_p clipped to +-limit_p where a limit is given
    num   = c + sum_p delta_p b_p
    den   = n + 2 sum_p delta_p Re h_p + sum_pq delta_p delta_q Re M_pq
    scale' = num / den
    score' = |num| / sqrt(den E)                        of the LINEARISED atom d + J delta (0 where E = 0)

(Nhat is evaluated as Re(M_pq - conj(h_p) h_q / n) / sqrt(M_pp M_qq); where |rho|^2 is zero or not finite -- an all-zero signal --
the quotient above is 0 / 0 and every pivot counts as not finite.)  A voxel is UNRESOLVED where `index` lies outside
`[0, natoms)`, -1 included, where `n` or an `M_pp` is zero or not finite, or where a Cholesky pivot of `Nhat` (the diagonal entry
before its root) is `<= rcond` or not finite.  `rcond` is a documented condition like `lstsq`'s: a pivot of 1e-10 means a Jacobian
column lies within 1e-5 rad of the span of `d` and the earlier columns.  An unresolved voxel gets NaN in every `delta_p`,
`scale' = rho` and `score'` = the unrefined score; where `index` is invalid scale 0 and score 0.  Never an error, and no atom
outside `[0, natoms)` is read.  A voxel's bits depend on its own signal, its atom's columns, nrec and the arguments only.
`refine_host` states the same formulas in NumPy on host arrays; it is the definition the tests hold, not a path of `refine`.

Mixtures (`Components`, `nnls`, csrc/epgx_nnls.hip through `epgx_signal_component_gram` / `epgx_signal_nnls`): everything above
takes a voxel as ONE atom.  Multi-component analysis (T2 spectra, myelin water fraction, partial volume) takes it as a
non-negative mixture of the atoms along one grid axis, the component axis, and chooses every other axis (B1, say) by the best fit,

    comp = match.Components(handle, axis=0)     # H_g and the validity masks, computed once, kept in HBM
    fit = match.nnls(comp, signals)             # .weights, .group, .residual, .status, .fraction(lo, hi, T2), .gmean(T2)

`D[t, a, g]`: records t, atoms a < A <= 64 along the component axis, groups g < G = every other grid axis flattened in C order;
`S[t, m]` the measured signals, complex128.  For every voxel m and group g

    H_g[a,b] = Re sum_t conj(D[t,a,g]) D[t,b,g]          (A x A, real symmetric; once per dictionary)
    f[a]     = Re sum_t conj(D[t,a,g]) S[t,m]            E = sum_t |S[t,m]|^2
    mu_g     = reg * (trace(H_g over the valid atoms) / (number of valid atoms))
    x*       = argmin over real x >= 0 of  J(x) = ||S[:,m] - sum_a x_a D[:,a,g]||^2 + mu_g ||x||^2
             = argmin over x >= 0 of  x^T (H_g + mu_g I) x - 2 f^T x + E

An atom is VALID where `H_g[a,a]` is finite and > 0 (match's rule); an invalid atom gets weight 0 and is never a candidate.  The
solver is Lawson and Hanson's active set on the Gram form: with x = 0 and an empty passive set P, the atom outside P with the
largest `w_a = f_a - ((H_g + mu_g I) x)_a` enters (the LOWEST a among equal w) while `w_a > tol sqrt(H_g[a,a] E)`; the passive
set is solved by Cholesky of `(H_g + mu_g I)[P,P]` in the order the atoms entered; while a solution s has an entry <= 0 the
iterate moves by `alpha = min x_p / (x_p - s_p)` over those entries towards s and the atoms that reach 0 leave.  In the end
`J = E - sum_a x_a (f_a + w_a)`.  Per voxel: the weights of the chosen group; the group (without `group=`: the g of the smallest
finite J, the LOWEST g among equal J); `residual = sqrt(max(J - mu_g ||x||^2, 0))`; `status` 0: solved, 1: the cap of 3 A
passive-set solves (scipy's) was reached and the weights are the last feasible iterate, 2: a pivot of the factorisation was not
finite or <= 0, or a sum (E, an f_a, an entry of a solution, J) was not finite -- the weights are NaN and the search skips the group.
Where every group is skipped: group -1, NaN weights, NaN residual, status 2.  An all-zero signal: weights 0, status 0, residual 0
in group 0.  Never an error.  A voxel's bits depend on its own signal, the dictionary and the arguments only.
The Gram form resolves the problem down to about sqrt(2^-53) only (the caveat of `compress`): `reg = 0` is for well-conditioned
dictionaries; the default 1e-8 bounds cond(H_g + mu_g I) by about A / reg and costs 1e-8 of the mean atom energy per unit weight.
`nnls_host` states the same method in NumPy on host arrays; it is the definition the tests hold, not a path of `nnls`.

The chi^2-driven ridge (`nnls(..., chi2=1.02)`, csrc/epgx_nnls_chi2.hip through `epgx_signal_nnls_chi2`): the fixed ridge `reg` is
there for the Cholesky factor, not for the spectrum, and the unregularised weights are the spiky minimum-support solution.
Multi-component T2 analysis (Whittall and MacKay; DECAES) raises the ridge until the data misfit has grown by a chosen factor and
reports the smooth spectrum there.  With `Jd(mu) = J - mu ||x(mu)||^2` the data misfit of the minimiser x(mu) >= 0 at the ridge mu:

    1. group and baseline: exactly the above at mu_0 = reg * mean valid H_g[a,a]; x_0, Jd_0 = Jd(mu_0).  The group never changes
       afterwards (the DECAES rule: the flip angle comes from the unregularised chi^2).  Status 1 and 2 pass through unchanged,
       with mu = mu_0, chi2 = 1 (both NaN at status 2) and evals = 0
    2. status 4 where Jd_0 <= 0 or Jd_0 < 4 * 8 (nrec + A) 2^-53 E / chi2_rtol: 8 (nrec + A) 2^-53 E is the rounding of the Gram-form
       J, below that floor the ratio cannot be resolved to chi2_rtol; x_0, mu = mu_0, chi2 = 1, evals = 0
    3. T = chi2 * Jd_0.  |Jd_0 / T - 1| <= chi2_rtol: status 0 at mu_0.  T >= E (no ridge reaches it: x = 0 has Jd = E): status 3 at mu_0
    4. r(mu) = Jd(mu) / T - 1, every evaluation one cold fit (x = 0, empty passive set) at its mu:
       bracket   mu = 16 mu_lo from mu_lo = mu_0 while r(mu) < -chi2_rtol
       Illinois  mu = mu_lo exp(r_lo / (r_lo - r_hi) log(mu_hi / mu_lo)); the new point replaces the end of its sign; where the
                 same end is replaced twice running, the r of the other end is halved
       |r(mu)| <= chi2_rtol: status 0, the weights at that mu.  After NNLS_CHI2_EVALS = 40 fits, at a fit that is not status 0
       or a mu that is not finite: status 3 with the evaluated point of the largest Jd <= T (the baseline if no other)

`Jd` is non-decreasing in mu for the constrained problem, so the root is bracketed from mu_0 upward.  `.mu` is the ridge of the
returned weights, `.chi2 = Jd / Jd_0`, `.evals` the fits of step 4, `.residual = sqrt(max(Jd, 0))`.  `nnls_host(..., chi2=)` is the
same search in NumPy (its exp and log are NumPy's, so a mu agrees with the device's to rounding, not to the bit).
"""
import numpy as np

__all__ = ["Dictionary", "MatchResult", "match", "Basis", "compress", "gram_basis", "select_rank", "MAX_RANK",
           "RefineResult", "refine", "refine_host", "MAX_REFINE_PARAMS", "Components", "NnlsResult", "nnls", "nnls_host",
           "MAX_COMPONENTS"]

MAX_RANK = 64          # basis vectors `epgx_signal_project` takes
MAX_REFINE_PARAMS = 4  # REFINE_MAX_P of csrc/epgx_refine.h
MAX_COMPONENTS = 64    # NNLS_MAX_A of csrc/epgx_nnls.h: one lane of a wavefront per atom of the component axis


def _dtype(dtype, name):
    """np.complex128 for None / complex128, np.complex64 for complex64; ValueError for anything else"""
    if dtype is None:
        return np.dtype(np.complex128)
    try:
        dt = np.dtype(dtype)
    except TypeError:
        dt = None
    if dt not in (np.dtype(np.complex128), np.dtype(np.complex64)):
        raise ValueError(f"{name}: dtype={dtype!r}; complex128 (None) or complex64")
    return dt


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


def _is_jacobian(arg):
    from . import functions
    return isinstance(arg, functions.DeviceJacobian)


class _Records:
    """complex128 records [nrec][ncol] on one device: a view of a DeviceSignal, or a host array uploaded into a buffer of its own;
    `narrowed()` gives the complex64 records (`dtype`), always in a buffer of their own"""

    dtype = np.dtype(np.complex128)

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

    def narrowed(self):
        """these records rounded once to complex64, dense rows: host records by `astype` (uploaded later at 8 bytes per element),
        device records by epgx_signal_narrow into a new buffer -- the source is only read and not kept"""
        from . import _lib
        out = object.__new__(_Records)
        out.nrec, out.shape, out.ncol, out.row_stride = self.nrec, self.shape, self.ncol, self.ncol
        out.dtype = np.dtype(np.complex64)
        if self.keep is None:
            with np.errstate(over="ignore"):             # (overflow goes to Inf, as on the device)
                out._host = self._host.astype(np.complex64)
            out.keep, out.ctx, out.device = None, None, None
        else:
            out.keep = _lib.signal_narrow(self.ctx, self.ptr, self.row_stride, self.nrec, self.ncol)
            out.ctx, out.device = self.ctx, self.device
        return out

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
    dtype: None / complex128, or complex64: the dictionary then owns a dense complex64 buffer `[nrec][natoms]` that holds the
    records rounded once (a handle is narrowed on the device and neither modified nor kept, an array by `astype` on the host).
    `.grid`, `.natoms`, `.nrec`, `.dtype`; `.norms` downloads `n_a` as float64 `grid`; `.download()` the records."""

    def __init__(self, handle, device=None, dtype=None):
        from . import _lib
        internal = isinstance(handle, _Records)
        want = handle.dtype if internal and dtype is None else _dtype(dtype, "dictionary")
        rec = handle if internal else _Records(handle, "dictionary")
        if len(rec.shape) == 0 and rec.keep is None:
            raise ValueError(f"dictionary: an array [nrec, *grid] with at least one grid axis, got shape ({rec.nrec},)")
        if rec.nrec < 1 or rec.ncol < 1:
            raise ValueError(f"dictionary: {rec.nrec} records of {rec.ncol} atoms; both must be at least 1")
        if want != rec.dtype:
            if want != np.complex64:
                raise NotImplementedError("dictionary: complex64 records are not widened to complex128")
            rec = rec.narrowed()
        if rec.keep is None:
            rec.upload(_lib.get_context(device))
        self._rec = rec
        self.grid, self.natoms, self.nrec, self.device, self.dtype = rec.shape, rec.ncol, rec.nrec, rec.device, rec.dtype
        self.basis = None          # the `Basis` of a dictionary that `compress` made
        self.jacobian = handle if _is_jacobian(handle) else None      # the DeviceJacobian it was built from (`refine`)
        self._norms = _lib.signal_norms(rec.ctx, rec.ptr, rec.row_stride, rec.nrec, rec.ncol, c64=self.dtype == np.complex64)

    @property
    def norms(self):
        return self._norms.download(np.float64, (self.natoms,)).reshape(self.grid)

    @property
    def records(self):
        """the records as a DeviceSignal `[nrec, *grid]` (np.asarray downloads them)"""
        from . import functions, _lib
        if self.dtype != np.complex128:
            raise NotImplementedError("records: a DeviceSignal holds complex128; download() returns the complex64 records")
        keep = self._rec.keep
        return functions.DeviceSignal(keep, self.nrec, self.grid, 0, 1) if isinstance(keep, _lib.DeviceBuffer) else keep

    def download(self):
        """the records as a NumPy array `[nrec, *grid]` of the dictionary's dtype"""
        if self.dtype == np.complex128:
            return np.asarray(self.records).reshape((self.nrec,) + self.grid)
        from . import _lib
        keep = self._rec.keep
        if not keep.ptr:
            raise _lib.EpgxError("download: the dictionary's buffer was freed")
        return keep.download(np.complex64, (self.nrec, self.natoms)).reshape((self.nrec,) + self.grid)

    def astype(self, dtype):
        """complex64 of a complex128 dictionary: a new `Dictionary` that owns the records rounded once on the device (`.basis` is
        carried along); the dictionary's own dtype: `self`; complex128 of a complex64 one: NotImplementedError"""
        want = _dtype(dtype, "astype")
        if want == self.dtype:
            return self
        if want == np.complex128:
            raise NotImplementedError("astype: a complex64 dictionary is not widened; build it from the complex128 records")
        out = Dictionary(self._rec.narrowed())
        out.basis = self.basis
        return out


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
    Returns a `MatchResult` whose arrays have the shape `signals.shape[1:]`.

    With a compressed dictionary (`compress(...).dictionary`, Dc = U^H D) the call is DEFINED as
    `match(Dictionary(U^H D), U^H S)`: signals with `basis.nrec` records are projected on the device first (`basis.project`),
    signals with `basis.rank` records are taken as projected already, any other record count raises ValueError (where rank =
    nrec both counts coincide and the signals count as not yet projected).  `score` is then relative to the energy of the
    PROJECTED signal, sum_r |Sc[r,m]|^2 -- the part of the signal outside the basis does not lower it.

    With a complex64 dictionary the signals are rounded once to complex64 (a host array by `astype`, a DeviceSignal on the
    device into a temporary) and matched in single precision (module docstring); signals that a compressed complex64 dictionary
    projects are projected in float64 first and rounded then.  Anything that is not a `Dictionary` is matched in complex128."""
    from . import _lib
    sig = _Records(signals, "signals")
    basis = dictionary.basis if isinstance(dictionary, Dictionary) else None
    if basis is not None:
        if sig.nrec != basis.nrec and sig.nrec != basis.rank:
            raise ValueError(f"signals: {sig.nrec} records; the compressed dictionary takes {basis.nrec} (projected on the device first) "
                             f"or {basis.rank} (projected already)")
        if sig.nrec == basis.nrec:
            rec = dictionary._rec
            if sig.device is not None and (sig.device != rec.device or sig.ctx is not rec.ctx):
                raise ValueError(f"signals: on device {sig.device}, the dictionary on device {rec.device}; both must be on one GPU (and context)")
            proj = basis._project(sig, rec.ctx)
            try:
                return _match_records(dictionary, _Records(proj, "signals"), nsplit)
            finally:
                proj._buf.free()        # (stream-ordered, as below)
    if not isinstance(dictionary, Dictionary):
        # (checked before the dictionary touches the device)
        probe = _Records(dictionary, "dictionary")
        if probe.nrec != sig.nrec:
            raise ValueError(f"signals: {sig.nrec} records, the dictionary has {probe.nrec}")
        if sig.device is not None and probe.device is not None and sig.device != probe.device:
            raise ValueError(f"signals: on device {sig.device}, the dictionary on device {probe.device}; both must be on one GPU")
        dictionary = Dictionary(probe, device=sig.device)
    return _match_records(dictionary, sig, nsplit)


def _match_records(dictionary, sig, nsplit):
    from . import _lib
    if dictionary.nrec != sig.nrec:
        raise ValueError(f"signals: {sig.nrec} records, the dictionary has {dictionary.nrec}")
    rec = dictionary._rec
    if sig.device is not None and (sig.device != rec.device or sig.ctx is not rec.ctx):
        raise ValueError(f"signals: on device {sig.device}, the dictionary on device {rec.device}; both must be on one GPU (and context)")
    c64 = dictionary.dtype == np.complex64
    if c64:
        sig = sig.narrowed()       # host records by astype; a handle on the device, into a temporary that is freed below
    sig.upload(rec.ctx)
    index, scale, score = _lib.signal_match(rec.ctx, rec.ptr, rec.row_stride, dictionary._norms.ptr.value if dictionary._norms.ptr else None,
                                            dictionary.natoms, sig.ptr, sig.row_stride, sig.nrec, sig.ncol, nsplit=nsplit, c64=c64)
    if isinstance(sig.keep, _lib.DeviceBuffer):
        sig.keep.free()        # (stream-ordered: the block is recycled behind the kernels that read it)
    return MatchResult(index.reshape(sig.shape), scale.reshape(sig.shape), score.reshape(sig.shape), dictionary.grid)


# ------------------------------------------------------------------------------------------------ SVD compression
def gram_basis(G):
    """the host half of `compress`: Gram matrix `[nrec, nrec]` -> `(U, lam)`, the eigenvectors (columns, complex128) and
    eigenvalues of `(G + G^H) / 2` by numpy.linalg.eigh, eigenvalues DESCENDING.  The gauge is fixed: every column is scaled by
    a unit phase so that its component of largest modulus (the lowest index among equal moduli) is real and positive -- U is a
    function of the bits of G"""
    G = np.asarray(G, dtype=np.complex128)
    if G.ndim != 2 or G.shape[0] != G.shape[1] or G.shape[0] < 1:
        raise ValueError(f"gram_basis: a square matrix, got shape {G.shape}")
    lam, U = np.linalg.eigh((G + G.conj().T) / 2)
    lam, U = lam[::-1].copy(), np.ascontiguousarray(U[:, ::-1])
    cols = np.arange(U.shape[1])
    k = np.argmax(np.abs(U), axis=0)                 # (the first among equal moduli)
    pivot = U[k, cols]
    U = U * (np.conj(pivot) / np.abs(pivot))[None, :]
    U[k, cols] = np.abs(pivot)                       # exactly real
    return U, lam


def resolved_rank(lam):
    """the number of leading eigenvalues the Gram route resolves: lam_r > nrec 2^-52 lam_0"""
    lam = np.asarray(lam, dtype=np.float64)
    if lam[0] <= 0:
        return 0
    return int(np.count_nonzero(lam > len(lam) * 2.0 ** -52 * lam[0]))


def select_rank(lam, rank=None, energy=None):
    """the rank `compress` keeps, from the descending eigenvalues: `rank` itself, or the smallest rank whose eigenvalues reach
    the share `energy` of trace(G).  ValueError where no eigenvalue is positive (no valid atom), the rank is outside
    1 .. min(MAX_RANK, nrec), `energy` needs more than MAX_RANK, or the rank reaches eigenvalues that are not resolved"""
    lam = np.asarray(lam, dtype=np.float64)
    nrec = len(lam)
    if (rank is None) == (energy is None):
        raise ValueError("compress: exactly one of rank= and energy= must be given")
    if not np.isfinite(lam).all() or lam[0] <= 0:
        raise ValueError("compress: the dictionary has no valid atom (every atom is all zero or holds a NaN / Inf)")
    if rank is not None:
        _check_rank(rank, nrec)
        rank = int(rank)
    else:
        share = np.cumsum(np.clip(lam, 0, None))
        share /= share[-1]
        rank = int(np.searchsorted(share, energy, side="left")) + 1
        if rank > min(MAX_RANK, nrec):
            raise ValueError(f"compress: energy={energy} needs rank {rank}; at most {MAX_RANK} basis vectors are supported "
                             f"(the first {min(MAX_RANK, nrec)} keep {share[min(MAX_RANK, nrec) - 1]:.12g})")
    most = resolved_rank(lam)
    if rank > most:
        raise ValueError(f"compress: rank {rank} reaches eigenvalues of the Gram matrix that are not resolved "
                         f"(lambda_r <= nrec 2^-52 lambda_0); the largest resolvable rank is {most}")
    return rank


def _check_rank(rank, nrec):
    if int(rank) != rank or not 1 <= rank <= MAX_RANK:
        raise ValueError(f"compress: rank={rank} not in 1 .. {MAX_RANK}")
    if rank > nrec:
        raise ValueError(f"compress: rank={rank} above the {nrec} records of the dictionary")


class Basis:
    """the temporal basis of a compressed dictionary.

    `U` complex128 `[nrec, rank]` (host), `s` the singular values sqrt(lambda) of the dictionary, all nrec of them, descending
    (negative lambda clipped to 0), `rank`, `nrec`, `energy` the share of trace(G) the rank keeps, `dictionary` the compressed
    `Dictionary` over `[rank, *grid]` in HBM (its `.basis` is this object)."""

    def __init__(self, U, lam, rank):
        lam = np.clip(np.asarray(lam, dtype=np.float64), 0, None)
        self.U = np.ascontiguousarray(U[:, :rank], dtype=np.complex128)
        self.s = np.sqrt(lam)
        self.nrec, self.rank = int(U.shape[0]), int(rank)
        self.energy = float(lam[:rank].sum() / lam.sum())
        self.dictionary = None
        self._dev = None             # (context, DeviceBuffer) of U

    def _device(self, ctx):
        from . import _lib
        if self._dev is None or self._dev[0] is not ctx:
            buf = _lib.DeviceBuffer(ctx, self.U.nbytes)
            buf.upload(self.U)
            self._dev = (ctx, buf)
        return self._dev[1]

    def _project(self, rec, ctx):
        """records `_Records` [nrec][ncol] -> DeviceSignal [rank, *shape] on `ctx`"""
        from . import _lib, functions
        rec.upload(ctx)
        ubuf = self._device(ctx)
        out = _lib.signal_project(ctx, ubuf.ptr.value if ubuf.ptr else None, self.rank, rec.ptr, rec.row_stride, self.nrec, rec.ncol)
        if isinstance(rec.keep, _lib.DeviceBuffer):
            rec.keep.free()          # (stream-ordered: the block is recycled behind the kernel that reads it)
        return functions.DeviceSignal(out, self.rank, rec.shape, 0, 1)

    def project(self, signals, device=None):
        """Sc[r, m] = sum_t conj(U[t, r]) S[t, m] on the device: signals NumPy `[nrec, *shape]` or a whole DeviceSignal ->
        DeviceSignal `[rank, *shape]`"""
        from . import _lib
        rec = _Records(signals, "signals")
        if rec.nrec != self.nrec:
            raise ValueError(f"signals: {rec.nrec} records, the basis has {self.nrec}")
        ctx = rec.ctx
        if ctx is None:
            ctx = self.dictionary._rec.ctx if self.dictionary is not None and device is None else _lib.get_context(device)
        return self._project(rec, ctx)


def compress(dictionary, rank=None, energy=None, *, nsplit=0, device=None, dtype=None):
    """SVD compression of a dictionary in HBM (module docstring): returns the `Basis`; `basis.dictionary` is the compressed
    `Dictionary` [rank, *grid] that `match` takes.

    dictionary: a `Dictionary`, or anything `Dictionary` takes (DeviceSignal, DeviceJacobian, NumPy array `[nrec, *grid]`).
    Exactly one of rank (1 .. 64, at most nrec) and energy (0 < energy <= 1: the smallest rank whose eigenvalues reach that
    share of trace(G)).  nsplit: ranges the Gram kernel cuts the atoms into (0: the library's rule, a function of nrec and
    natoms alone, so that the same dictionary gives the same basis on every machine).
    ValueError: rank above 64 or nrec, an energy that needs more than 64, a rank that reaches unresolved eigenvalues
    (lambda_r <= nrec 2^-52 lambda_0), a dictionary without a valid atom.
    dtype=np.complex64: `basis.dictionary` is the projected dictionary rounded once to complex64 (the complex128 intermediate is
    freed); Gram matrix, eigenvectors and projection stay float64, `basis.U`, `basis.s`, `basis.energy` keep their bits.  A
    complex64 INPUT dictionary raises NotImplementedError (no single-precision Gram matrix).
    Only G (16 nrec^2 bytes) comes down and U (16 nrec rank bytes) goes up; the dictionary does not move."""
    from . import _lib, functions
    want = _dtype(dtype, "compress")
    if isinstance(dictionary, Dictionary) and dictionary.dtype != np.complex128:
        raise NotImplementedError("compress: a complex64 dictionary; the Gram matrix is taken in float64 -- compress the complex128 "
                                  "dictionary with dtype=np.complex64")
    if (rank is None) == (energy is None):
        raise ValueError("compress: exactly one of rank= and energy= must be given")
    if energy is not None and not 0.0 < energy <= 1.0:
        raise ValueError(f"compress: energy={energy} not in (0, 1]")
    if not isinstance(dictionary, Dictionary):
        probe = _Records(dictionary, "dictionary")      # (sharded and slab handles raise here, before the device)
        if rank is not None:
            _check_rank(rank, probe.nrec)
        dictionary = Dictionary(probe, device=device)
    elif rank is not None:
        _check_rank(rank, dictionary.nrec)
    rec = dictionary._rec
    ctx = rec.ctx
    gbuf = _lib.signal_gram(ctx, rec.ptr, rec.row_stride, dictionary._norms.ptr.value if dictionary._norms.ptr else None,
                            dictionary.nrec, dictionary.natoms, nsplit=nsplit)
    try:
        G = gbuf.download(np.complex128, (dictionary.nrec, dictionary.nrec))
    finally:
        gbuf.free()
    U, lam = gram_basis(G)
    basis = Basis(U, lam, select_rank(lam, rank, energy))
    ubuf = basis._device(ctx)
    out = _lib.signal_project(ctx, ubuf.ptr.value, basis.rank, rec.ptr, rec.row_stride, dictionary.nrec, dictionary.natoms)
    cdic = Dictionary(functions.DeviceSignal(out, basis.rank, dictionary.grid, 0, 1))
    if want == np.complex64:
        wide, cdic = cdic, cdic.astype(np.complex64)
        wide._norms.free()          # (stream-ordered: the blocks are recycled behind the kernel that narrowed them)
        out.free()
    cdic.basis, basis.dictionary = basis, cdic
    return basis


# ------------------------------------------------------------------------------------------------ Gauss-Newton refinement
class RefineResult:
    """`delta` float64 `[*shape, P]` (NaN where unresolved), `scale` complex128 and `score` float64 of the linearised atom, `index`
    int64 (the atoms the step started from), all over the shape of the measured voxels; `variables` the P chosen columns, `grid`
    the dictionary's grid"""

    def __init__(self, delta, scale, score, index, variables, grid):
        self.delta, self.scale, self.score, self.index = delta, scale, score, index
        self.variables, self.grid = list(variables), tuple(grid)

    def estimate(self, values):
        """the refined parameters `values[p][index] + delta[..., p]` as float64 `[*shape, P]`, NaN where unresolved.
        values: P arrays, each broadcastable to the grid, that hold the parameter of every atom (in the order of `variables`)"""
        values = list(values)
        if len(values) != len(self.variables):
            raise ValueError(f"estimate: {len(values)} arrays of values for the {len(self.variables)} variables {self.variables}")
        none = (self.index < 0) | (self.index >= int(np.prod(self.grid, dtype=np.int64)))
        at = np.where(none, 0, self.index)
        out = np.empty(self.delta.shape, dtype=np.float64)
        for p, val in enumerate(values):
            flat = np.broadcast_to(np.asarray(val, dtype=np.float64), self.grid).reshape(-1)
            out[..., p] = np.where(none, np.nan, flat[at]) + self.delta[..., p]
        return out


def _refine_limit(limit, nparam):
    """limit as float64 [nparam] of positive numbers (a scalar holds for every column, None entries and +Inf: no limit), or None"""
    if limit is None:
        return None
    if np.ndim(limit) == 0:
        limit = [limit] * nparam
    lim = np.array([np.inf if v is None else v for v in limit], dtype=np.float64)
    if lim.shape != (nparam,):
        raise ValueError(f"limit: {lim.shape[0] if lim.ndim == 1 else lim.shape} values for {nparam} variables")
    if not np.all(lim > 0):
        raise ValueError(f"limit: {lim.tolist()}; every limit must be positive (None or inf for none)")
    return lim


def _refine_rcond(rcond):
    if np.ndim(rcond) != 0 or not 0.0 <= float(rcond) < 1.0:
        raise ValueError(f"rcond: {rcond!r} not in [0, 1)")
    return float(rcond)


def _refine_index(result, shape, grid, natoms):
    """the atoms as int64 of the signals' shape, from a MatchResult or an int array; ValueError for values < -1 or >= natoms"""
    if isinstance(result, (MatchResult, RefineResult)):
        if tuple(result.grid) != tuple(grid):
            raise ValueError(f"result: matched against the grid {tuple(result.grid)}, the dictionary has {tuple(grid)}")
        result = result.index
    idx = np.asarray(result)
    if idx.dtype.kind not in "iu":
        raise ValueError(f"result: a MatchResult or an array of integer indices, got {idx.dtype}")
    if idx.shape != tuple(shape):
        raise ValueError(f"result: indices of shape {idx.shape}, the signals have {tuple(shape)}")
    idx = np.ascontiguousarray(idx, dtype=np.int64)
    if idx.size and (idx.min() < -1 or idx.max() >= natoms):
        raise ValueError(f"result: indices in [{idx.min()}, {idx.max()}]; -1 (no atom) .. {natoms - 1} are valid")
    return idx


def _refine_columns(variables, known):
    """positions in `known` of the chosen `variables` (None: all), 1 .. MAX_REFINE_PARAMS of them, each once"""
    chosen = list(known) if variables is None else list(variables)
    for v in chosen:
        if v not in known:
            raise ValueError(f"variables: {v!r} is not a column of the Jacobian, {list(known)}")
    if len(set(map(repr, chosen))) != len(chosen):
        raise ValueError(f"variables: {chosen} names a column twice")
    if not 1 <= len(chosen) <= MAX_REFINE_PARAMS:
        raise NotImplementedError(f"variables: {len(chosen)} columns; refine takes 1 .. {MAX_REFINE_PARAMS} -- choose them with "
                                  "variables=, or download the Jacobian (np.asarray) and use refine_host for more")
    return chosen, [list(known).index(v) for v in chosen]


def _refine_source(dictionary, jacobian):
    """the DeviceJacobian behind `dictionary`, or None for host arrays; raises for what `refine` does not take"""
    from . import functions
    if isinstance(dictionary, Dictionary):
        if dictionary.basis is not None:
            raise NotImplementedError("dictionary: a compressed dictionary holds no derivative rows; refine on the uncompressed "
                                      "DeviceJacobian with the indices of the compressed match")
        if dictionary.dtype != np.complex128:
            raise NotImplementedError("dictionary: a complex64 dictionary; refine runs in float64 on the complex128 DeviceJacobian "
                                      "-- pass that (the indices of a complex64 match are valid for it)")
        if dictionary.jacobian is None:
            raise ValueError("dictionary: this Dictionary was not built from a DeviceJacobian and holds no derivative rows")
        dictionary = dictionary.jacobian
    if isinstance(dictionary, functions.ShardedDeviceSignal):
        raise NotImplementedError("dictionary: a ShardedDeviceSignal (a run over several GPUs); refine takes the DeviceJacobian of a "
                                  "run on one GPU -- download it (np.asarray) or simulate the dictionary on one device")
    if isinstance(dictionary, functions.DeviceHessian):
        raise NotImplementedError("dictionary: a DeviceHessian holds second derivatives; refine takes the DeviceJacobian of the run "
                                  "(probe=epg.Jacobian([...]))")
    if isinstance(dictionary, functions.DeviceSignal):
        raise ValueError("dictionary: a DeviceSignal holds no derivative rows; simulate with probe=epg.Jacobian([...]) or pass host "
                         "arrays with jacobian=")
    if isinstance(dictionary, functions.DeviceJacobian):
        if jacobian is not None:
            raise ValueError("jacobian=: goes with a dictionary on the host; a DeviceJacobian brings its own derivative rows")
        return dictionary
    if jacobian is None:
        raise ValueError("jacobian=: a dictionary on the host needs its derivatives, a NumPy array [nrec, *grid, P]")
    return None


def refine(dictionary, signals, result, *, jacobian=None, variables=None, limit=None, rcond=1e-10):
    """one Gauss-Newton step off the grid at the matched atom of every measured voxel (module docstring), on the device.

    dictionary: a `DeviceJacobian`; a `Dictionary` built from one (its `.jacobian`); or a NumPy array `[nrec, *grid]` together
    with jacobian= NumPy `[nrec, *grid, P]` -- the two are uploaded once into one buffer in the `[record][row][atom]` layout.
    signals: as for `match`.  result: the `MatchResult` of these signals, or an int array of their shape (flat atom indices, -1:
    none); a value < -1 or >= natoms raises ValueError.
    variables: the columns to step in, a subset of the handle's `variables` in any order (host arrays: of 0 .. P - 1); default
    all of them -- "magnitude" apart, which is the probed state itself (the complex scale carries it) and raises ValueError
    when named.  1 .. 4, else NotImplementedError.  limit: None, one positive number, or one per variable (None / inf: no
    limit): |delta_p| <= limit_p.  rcond: the smallest Cholesky pivot of the equilibrated matrix that counts as resolved.
    The index goes up at 8 bytes per voxel and 8 P + 24 bytes per voxel come back; dictionary and Jacobian do not move.
    NotImplementedError, naming the way out, for a compressed or complex64 `Dictionary`, a ShardedDeviceSignal, a DeviceHessian.
    Returns a `RefineResult`."""
    from . import _lib
    handle = _refine_source(dictionary, jacobian)
    rcond = _refine_rcond(rcond)
    sig = _Records(signals, "signals")
    if handle is not None:
        # (a column at row 0, "magnitude", is the probed state itself: rho carries it already and the step leaves it out)
        known = list(handle.variables)
        chosen, cols = _refine_columns([v for v, r in zip(known, handle.rows) if r > 0] if variables is None else variables, known)
        rows = [handle.rows[c] for c in cols]
        if 0 in rows:
            raise ValueError(f"variables: {chosen[rows.index(0)]!r} is the probed state itself, not a derivative; the complex scale "
                             "of the result carries it")
        nrec, grid, natoms = handle.nrec, tuple(handle.grid), handle.nvox
    else:
        D, J = np.asarray(dictionary), np.asarray(jacobian)
        if D.ndim < 2 or D.dtype.kind not in "fciub" or J.dtype.kind not in "fciub" or J.shape[:-1] != D.shape:
            raise ValueError(f"dictionary [nrec, *grid] and jacobian [nrec, *grid, P]: got shapes {D.shape} and {J.shape}")
        if 0 in J.shape:
            raise ValueError(f"jacobian: shape {J.shape}; records, atoms and columns must be at least 1 each")
        chosen, cols = _refine_columns(variables, list(range(J.shape[-1])))
        rows = [1 + p for p in range(len(cols))]
        nrec, grid = D.shape[0], tuple(D.shape[1:])
        natoms = int(np.prod(grid, dtype=np.int64))
    if sig.nrec != nrec:
        raise ValueError(f"signals: {sig.nrec} records, the dictionary has {nrec}")
    lim = _refine_limit(limit, len(chosen))
    index = _refine_index(result, sig.shape, grid, natoms)

    if handle is not None:
        buf = handle._buf
        ctx = buf.ctx
        if sig.device is not None and (sig.device != handle.device or sig.ctx is not ctx):
            raise ValueError(f"signals: on device {sig.device}, the dictionary on device {handle.device}; both must be on one GPU (and context)")
        # (a handle whose buffer was freed hands over NULL: the library's EpgxError, as for a download)
        own, ptr, record_stride, row_stride, nrow = None, handle.ptr if buf.ptr else None, handle.record_stride, handle.row_stride, handle._nrow
    else:
        ctx = sig.ctx if sig.ctx is not None else _lib.get_context(None)
        host = np.empty((nrec, 1 + len(cols), natoms), dtype=np.complex128)
        host[:, 0] = D.reshape(nrec, natoms)
        host[:, 1:] = np.moveaxis(J.reshape(nrec, natoms, -1)[:, :, cols], 2, 1)
        own = _lib.DeviceBuffer(ctx, host.nbytes)
        own.upload(host)
        ptr, record_stride, row_stride, nrow = own.ptr.value, (1 + len(cols)) * natoms, natoms, 1 + len(cols)
    sig.upload(ctx)
    try:
        delta, scale, score = _lib.signal_refine(ctx, ptr, record_stride, row_stride, nrow, nrec, rows, natoms, sig.ptr, sig.row_stride,
                                                 sig.ncol, index.reshape(-1), limit=lim, rcond=rcond)
    finally:
        if isinstance(sig.keep, _lib.DeviceBuffer):
            sig.keep.free()        # (stream-ordered: the block is recycled behind the kernel that reads it)
        if own is not None:
            own.free()
    return RefineResult(np.ascontiguousarray(delta.T).reshape(sig.shape + (len(chosen),)), scale.reshape(sig.shape).copy(),
                        score.reshape(sig.shape).copy(), index, chosen, grid)


def refine_host(D, J, S, index, limit=None, rcond=1e-10):
    """the formulas of `refine` (module docstring) in NumPy float64 on host arrays: the documented definition.  Not a path of
    `refine`, which never calls it.

    D `[nrec, *grid]`, J `[nrec, *grid, P]` (any P), S `[nrec, *shape]`, index int `[*shape]` (values outside [0, natoms) come
    back unresolved), limit and rcond as for `refine`.  Returns a `RefineResult` (`variables` = 0 .. P - 1)."""
    D, J, S = np.asarray(D, dtype=np.complex128), np.asarray(J, dtype=np.complex128), np.asarray(S, dtype=np.complex128)
    if D.ndim < 2 or J.shape[:-1] != D.shape or S.ndim < 1 or S.shape[0] != D.shape[0]:
        raise ValueError(f"refine_host: D [nrec, *grid], J [nrec, *grid, P], S [nrec, *shape]: got {D.shape}, {J.shape}, {S.shape}")
    nrec, grid, shape, P = D.shape[0], D.shape[1:], S.shape[1:], J.shape[-1]
    natoms = int(np.prod(grid, dtype=np.int64))
    idx = np.asarray(index, dtype=np.int64)
    if idx.shape != shape:
        raise ValueError(f"refine_host: indices of shape {idx.shape}, the signals have {shape}")
    lim = _refine_limit(limit, P)
    rcond = _refine_rcond(rcond)
    flat = idx.reshape(-1)
    valid = (flat >= 0) & (flat < natoms)
    at = np.where(valid, flat, 0)
    d = D.reshape(nrec, natoms)[:, at]                         # [nrec, nmeas]
    j = J.reshape(nrec, natoms, P)[:, at, :]                   # [nrec, nmeas, P]
    s = S.reshape(nrec, -1)
    with np.errstate(all="ignore"):
        n = (d.real ** 2 + d.imag ** 2).sum(axis=0)
        E = (s.real ** 2 + s.imag ** 2).sum(axis=0)
        c = (np.conj(d) * s).sum(axis=0)
        b = np.einsum("tmp,tm->mp", np.conj(j), s)
        h = np.einsum("tm,tmp->mp", np.conj(d), j)
        M = np.einsum("tmp,tmq->mpq", np.conj(j), j).real
        rho = c / n
        rho2 = rho.real ** 2 + rho.imag ** 2
        score0 = np.where(E == 0, 0.0, np.abs(c) / (np.sqrt(n) * np.sqrt(E)))
        mpp = np.einsum("mpp->mp", M)
        ok = valid & (n > 0) & np.isfinite(n) & (rho2 > 0) & np.isfinite(rho2) & np.all((mpp > 0) & np.isfinite(mpp), axis=1)
        sd = np.sqrt(mpp)
        A = M - (np.conj(h)[:, :, None] * h[:, None, :]).real / n[:, None, None]
        L = A / (sd[:, :, None] * sd[:, None, :])               # Nhat, factored in place below (lower triangle)
        y = (np.conj(rho)[:, None] * (b - rho[:, None] * np.conj(h))).real
        z = y / (rho2[:, None] * sd)
        for q in range(P):
            piv = L[:, q, q] - (L[:, q, :q] ** 2).sum(axis=1)
            ok &= (piv > rcond) & np.isfinite(piv)
            L[:, q, q] = np.sqrt(piv)
            for p in range(q + 1, P):
                L[:, p, q] = (L[:, p, q] - (L[:, p, :q] * L[:, q, :q]).sum(axis=1)) / L[:, q, q]
        for p in range(P):
            z[:, p] = (z[:, p] - (L[:, p, :p] * z[:, :p]).sum(axis=1)) / L[:, p, p]
        for p in range(P - 1, -1, -1):
            z[:, p] = (z[:, p] - (L[:, p + 1:, p] * z[:, p + 1:]).sum(axis=1)) / L[:, p, p]
        delta = z / sd
        if lim is not None:
            delta = np.where(delta > lim, lim, np.where(delta < -lim, -lim, delta))
        num = c + (delta * b).sum(axis=1)
        den = n + 2 * (delta * h.real).sum(axis=1) + np.einsum("mp,mq,mpq->m", delta, delta, M)
        scale = np.where(ok, num / den, rho)
        score = np.where(ok, np.where(E == 0, 0.0, np.abs(num) / (np.sqrt(den) * np.sqrt(E))), score0)
    delta = np.where(ok[:, None], delta, np.nan)
    scale = np.where(valid, scale, 0.0)
    score = np.where(valid, score, 0.0)
    return RefineResult(delta.reshape(shape + (P,)), scale.reshape(shape), score.reshape(shape), idx, list(range(P)), grid)


# ------------------------------------------------------------------------------------------------ non-negative mixtures
NNLS_REG = 1e-8        # default reg of `nnls`
NNLS_TOL = 1e-10       # default tol of `nnls`
NNLS_CHI2_RTOL = 1e-3  # default chi2_rtol of `nnls`
NNLS_CHI2_FACTOR = 16.0  # NNLS_CHI2_FACTOR of csrc/epgx_nnls.h: the step of the bracket
NNLS_CHI2_EVALS = 40     # NNLS_CHI2_EVALS of csrc/epgx_nnls.h: the fits a voxel's search may take


def _component_axis(axis, grid):
    """`axis` as an index into `grid` (negative from the end) -> (axis, A, nouter, ninner, groups)"""
    if isinstance(axis, (bool, np.bool_)) or int(axis) != axis or not -len(grid) <= axis < len(grid):
        raise ValueError(f"axis: {axis!r} is not an axis of the grid {tuple(grid)}")
    axis = int(axis) % len(grid)
    nouter = int(np.prod(grid[:axis], dtype=np.int64))
    ninner = int(np.prod(grid[axis + 1:], dtype=np.int64))
    return axis, int(grid[axis]), nouter, ninner, tuple(grid[:axis]) + tuple(grid[axis + 1:])


def _check_ncomp(A):
    if not 1 <= A <= MAX_COMPONENTS:
        raise NotImplementedError(f"axis: {A} atoms along the component axis; nnls takes 1 .. {MAX_COMPONENTS} (one lane of a wavefront "
                                  "each) -- thin the axis, or download the dictionary (np.asarray) and use nnls_host")


def _nnls_reg_tol(reg, tol):
    if np.ndim(reg) != 0 or not 0.0 <= float(reg) < np.inf:
        raise ValueError(f"reg: {reg!r} is not a finite number >= 0")
    if np.ndim(tol) != 0 or not 0.0 <= float(tol) < np.inf:
        raise ValueError(f"tol: {tol!r} is not a finite number >= 0")
    return float(reg), float(tol)


def _nnls_chi2(chi2, chi2_rtol, reg):
    """(chi2, chi2_rtol) as floats; chi2 None: (None, None)"""
    if chi2 is None:
        return None, None
    if np.ndim(chi2) != 0 or isinstance(chi2, (bool, np.bool_)) or not 1.0 < float(chi2) < np.inf:
        raise ValueError(f"chi2: {chi2!r} is not a finite number > 1 (the factor by which the data misfit may grow), or None")
    if np.ndim(chi2_rtol) != 0 or isinstance(chi2_rtol, (bool, np.bool_)) or not 0.0 < float(chi2_rtol) < 1.0:
        raise ValueError(f"chi2_rtol: {chi2_rtol!r} is not a number in (0, 1)")
    if not reg > 0.0:
        raise ValueError(f"reg: {reg!r} with chi2=: the search for the ridge grows from mu_0 = reg * mean H_aa and needs reg > 0")
    return float(chi2), float(chi2_rtol)


def _nnls_group(group, shape):
    """group= as int64 of the signals' shape, or None"""
    if group is None:
        return None
    grp = np.asarray(group)
    if grp.dtype.kind not in "iu":
        raise ValueError(f"group: an array of integer group indices, got {grp.dtype}")
    if grp.shape != tuple(shape):
        raise ValueError(f"group: indices of shape {grp.shape}, the signals have {tuple(shape)}")
    return np.ascontiguousarray(grp, dtype=np.int64)


class Components:
    """a dictionary on the device read as `D[t, a, g]` (module docstring): atoms a along the grid axis `axis`, groups g = every
    other axis flattened in C order, with its Gram matrices `H_g` and validity masks (computed once, kept in HBM next to the
    records, as `Dictionary` keeps its norms).

    handle: what `Dictionary` takes as complex128 -- a whole DeviceSignal, a DeviceJacobian (its probed-state row), a NumPy array
    `[nrec, *grid]` (uploaded once) -- or a complex128, uncompressed `Dictionary`.  axis: an index into `grid`, negative from the
    end; ANY axis: the kernels take its stride and the dictionary is not copied.
    `.grid`, `.axis`, `.ncomp` (A), `.groups` (the grid without the axis), `.ngroups` (G), `.nrec`; `.gram` downloads `H` as
    float64 `[G, A, A]`, `.valid` the masks as bool `[G, A]`.
    NotImplementedError, naming the way out: more than 64 atoms along the axis, a ShardedDeviceSignal or a voxel slab, a
    DeviceHessian, a complex64 or compressed `Dictionary`."""

    def __init__(self, handle, axis, *, device=None):
        from . import _lib
        if isinstance(handle, Dictionary):
            if handle.basis is not None:
                raise NotImplementedError("components: a compressed dictionary; its records are coefficients of a temporal basis and "
                                          "the mixture is fitted to the records themselves -- pass the uncompressed handle")
            if handle.dtype != np.complex128:
                raise NotImplementedError("components: a complex64 dictionary; nnls runs in float64 on the complex128 records "
                                          "-- pass the handle the dictionary was narrowed from")
            rec = handle._rec
        else:
            rec = _Records(handle, "components")
        if len(rec.shape) == 0:
            raise ValueError(f"components: an array [nrec, *grid] with at least one grid axis, got shape ({rec.nrec},)")
        if rec.nrec < 1 or rec.ncol < 1:
            raise ValueError(f"components: {rec.nrec} records of {rec.ncol} atoms; both must be at least 1")
        self.axis, self.ncomp, self._nouter, self._ninner, self.groups = _component_axis(axis, rec.shape)
        _check_ncomp(self.ncomp)
        if rec.keep is None:
            rec.upload(_lib.get_context(device))
        self._rec = rec
        self.grid, self.nrec, self.device = rec.shape, rec.nrec, rec.device
        self.ngroups = self._nouter * self._ninner
        self._gram, self._mask = _lib.signal_component_gram(rec.ctx, rec.ptr, rec.row_stride, rec.nrec, self.ncomp, self._ninner,
                                                            self._nouter, self._ninner)

    @property
    def gram(self):
        return self._gram.download(np.float64, (self.ngroups, self.ncomp, self.ncomp))

    @property
    def valid(self):
        bits = self._mask.download(np.uint64, (self.ngroups,))
        return ((bits[:, None] >> np.arange(self.ncomp, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(bool)


class NnlsResult:
    """`weights` float64 `[A, *shape]` (>= 0; NaN where no group could be solved), `group` int64 `shape` (flat index into `groups`,
    -1: none), `residual` float64 (the norm of the data misfit), `status` int32 (0 solved, 1 iteration cap, 2 not solved), all
    over the shape of the measured voxels; `groups` the dictionary's grid without the component axis.  `nnls_host` adds `solves`
    (passive-set solves) and `left` (atoms that left the passive set) of the chosen group, int64; None from the device.
    With `chi2=` (module docstring; None without): `mu` float64, the absolute ridge at which the returned weights were solved,
    `chi2` float64, the achieved ratio Jd(mu) / Jd(mu_0), `evals` int32, the fits the search took; `status` 3: the search ended
    without meeting `chi2_rtol`, 4: the misfit lies below the resolution of the Gram form and nothing was regularised; `solves` and
    `left` are those of the baseline fit."""

    def __init__(self, weights, group, residual, status, groups, solves=None, left=None, mu=None, chi2=None, evals=None):
        self.weights, self.group, self.residual, self.status, self.groups = weights, group, residual, status, tuple(groups)
        self.solves, self.left = solves, left
        self.mu, self.chi2, self.evals = mu, chi2, evals

    def unravel(self):
        """tuple of index arrays, one per axis of `groups` (np.unravel_index); -1 stays -1 on every axis"""
        if not self.groups:
            return ()
        none = self.group < 0
        axes = np.unravel_index(np.where(none, 0, self.group), self.groups)
        return tuple(np.where(none, -1, ax) for ax in axes)

    def _values(self, values, what):
        v = np.asarray(values, dtype=np.float64)
        if v.shape != (self.weights.shape[0],):
            raise ValueError(f"{what}: {v.shape} values for the {self.weights.shape[0]} atoms of the component axis")
        return v.reshape((-1,) + (1,) * (self.weights.ndim - 1))

    def fraction(self, lo, hi, values):
        """the share of the weights whose `values[a]` lie in `[lo, hi)`: sum over those / sum over all; NaN where that sum is 0"""
        v = self._values(values, "fraction")
        with np.errstate(invalid="ignore", divide="ignore"):
            total = self.weights.sum(axis=0)
            return np.where(total == 0, np.nan, (self.weights * ((v >= lo) & (v < hi))).sum(axis=0) / total)

    def gmean(self, values):
        """the weighted geometric mean `exp(sum_a w_a log values[a] / sum_a w_a)`; NaN where the sum of the weights is 0"""
        v = self._values(values, "gmean")
        with np.errstate(invalid="ignore", divide="ignore"):
            total = self.weights.sum(axis=0)
            return np.where(total == 0, np.nan, np.exp((self.weights * np.log(v)).sum(axis=0) / total))


def nnls(components, signals, *, reg=NNLS_REG, tol=NNLS_TOL, group=None, chi2=None, chi2_rtol=NNLS_CHI2_RTOL, _max_evals=None):
    """non-negative mixture of the atoms along the component axis for every measured voxel and the best group (module
    docstring), on the device: `nnls_kernel` of csrc/epgx_nnls.hip, one wavefront per voxel, one lane per atom.

    components: a `Components`.  signals: as for `match` (a NumPy array `[nrec, *shape]`, real or complex, or a whole DeviceSignal
    on the dictionary's device and context).
    reg >= 0: the ridge `mu_g = reg * mean valid H_g[a,a]`.  Default 1e-8: the Gram form squares the condition of the dictionary,
    and 1e-8 of the mean atom energy bounds cond(H_g + mu_g I) by about A / reg ~ 1e10, which float64 Cholesky resolves, while
    it moves the objective by at most 1e-8 ||x||^2 mean|D_a|^2; reg = 0 is for well-conditioned dictionaries.
    tol >= 0: an atom outside the passive set enters only while `w_a > tol sqrt(H_g[a,a] E)`.  By Cauchy-Schwarz
    `w_a / sqrt(H_g[a,a] E)` is at most the cosine between atom and residual times |residual| / |signal|, in [-1, 1]; w_a is
    evaluated from the Gram form with an error of about A 2^-53 sqrt(cond) on that scale, 1e-14 .. 1e-12.  The default 1e-10
    stands two orders above that noise, so no atom enters on rounding alone (which would cycle up to the cap), and an atom left
    out at w_a <= tol sqrt(H_aa E) could lower J by w_a^2 / H_aa <= tol^2 E = 1e-20 E at most: far below what float64 shows.
    group: None (search all groups), or an int array of the signals' shape that fixes each voxel's group, a binned B1 map say; an
    entry outside [0, G) gives that voxel group -1, NaN weights, NaN residual and status 2, and reads nothing.
    chi2: None, or a finite number > 1: the chi^2-driven ridge of the module docstring -- after the fit above (which fixes the
    group), `nnls_chi2_kernel` of csrc/epgx_nnls_chi2.hip raises the ridge of every voxel from mu_0 until the data misfit is
    `chi2` times that of the unregularised fit within `chi2_rtol` (in (0, 1)), and the smooth weights at that ridge come back
    with `.mu`, `.chi2`, `.evals` and the statuses 3 and 4.  1.02 is the convention of myelin water imaging.  Needs reg > 0.
    The group goes from one kernel to the next in device memory.
    A 8 + 20 bytes per voxel come back (A 8 + 40 with chi2=); the dictionary does not move.  Returns an `NnlsResult`."""
    from . import _lib
    if not isinstance(components, Components):
        raise ValueError("components: a match.Components (the dictionary with its component axis chosen)")
    reg, tol = _nnls_reg_tol(reg, tol)
    chi2, chi2_rtol = _nnls_chi2(chi2, chi2_rtol, reg)
    sig = _Records(signals, "signals")
    if sig.nrec != components.nrec:
        raise ValueError(f"signals: {sig.nrec} records, the dictionary has {components.nrec}")
    rec = components._rec
    if sig.device is not None and (sig.device != rec.device or sig.ctx is not rec.ctx):
        raise ValueError(f"signals: on device {sig.device}, the dictionary on device {rec.device}; both must be on one GPU (and context)")
    grp = _nnls_group(group, sig.shape)
    sig.upload(rec.ctx)
    args = (rec.ctx, rec.ptr, rec.row_stride, components.nrec, components.ncomp, components._ninner, components._nouter,
            components._ninner, components._gram.ptr.value if components._gram.ptr else None,
            components._mask.ptr.value if components._mask.ptr else None, sig.ptr, sig.row_stride, sig.ncol, reg, tol)
    extra = ()
    try:
        if chi2 is None:
            weights, chosen, residual, status = _lib.signal_nnls(*args, None if grp is None else grp.reshape(-1))
        else:
            weights, chosen, residual, status, *extra = _lib.signal_nnls_chi2(
                *args, chi2, chi2_rtol, None if grp is None else grp.reshape(-1),
                _lib.NNLS_CHI2_EVALS if _max_evals is None else _max_evals)
    finally:
        if isinstance(sig.keep, _lib.DeviceBuffer):
            sig.keep.free()        # (stream-ordered: the block is recycled behind the kernel that reads it)
    return NnlsResult(weights.reshape((components.ncomp,) + sig.shape).copy(), chosen.reshape(sig.shape).copy(),
                      residual.reshape(sig.shape).copy(), status.reshape(sig.shape).copy(), components.groups,
                      **{k: v.reshape(sig.shape).copy() for k, v in zip(("mu", "chi2", "evals"), extra)})


def _nnls_task(H, valid, mu, f, E, tol, cap=None):
    """one (voxel, group) of `nnls_host`: H [A, A] without the ridge, valid bool [A], f [A], E -> (x, J, J_data, status, solves, left);
    cap: the passive-set solves allowed, 3 A (a test lowers it)"""
    A = len(f)
    cap = 3 * A if cap is None else cap
    nan = np.full(A, np.nan)
    diag = np.where(valid, np.diagonal(H), 0.0)
    if not np.isfinite(E) or not np.isfinite(f[valid]).all():
        return nan, np.nan, np.nan, 2, 0, 0
    Hm = H + mu * np.eye(A)
    thr = tol * np.sqrt(diag * E)
    x, w, P = np.zeros(A), np.where(valid, f, 0.0), []
    status, solves, left = 0, 0, 0

    def gradient():
        out = f.copy()
        for p in P:                                    # in the order the atoms entered
            out = out - np.where(valid, Hm[p], 0.0) * x[p]
        return np.where(valid, out, 0.0)

    while status == 0:
        cand = valid & (w > thr)
        cand[P] = False
        if not cand.any():
            break
        P.append(int(np.argmax(np.where(cand, w, -np.inf))))       # (the first among equal w)
        while True:
            if solves == cap:
                status = 1
                break
            solves += 1
            k = len(P)
            L = np.zeros((k, k))
            for q in range(k):
                for i in range(q):
                    L[q, i] = (Hm[P[q], P[i]] - L[q, :i] @ L[i, :i]) / L[i, i]
                piv = Hm[P[q], P[q]] - L[q, :q] @ L[q, :q]
                if not (np.isfinite(piv) and piv > 0):
                    return nan, np.nan, np.nan, 2, solves, left
                L[q, q] = np.sqrt(piv)
            s = f[P].copy()
            for q in range(k):
                s[q] = (s[q] - L[q, :q] @ s[:q]) / L[q, q]
            for q in range(k - 1, -1, -1):
                s[q] = (s[q] - L[q + 1:, q] @ s[q + 1:]) / L[q, q]
            if not np.isfinite(s).all():
                return nan, np.nan, np.nan, 2, solves, left
            xp = x[P]
            neg = ~(s > 0)
            if not neg.any():
                x[:] = 0.0
                x[P] = s
                break
            with np.errstate(invalid="ignore", divide="ignore"):
                al = np.where(neg, np.where(xp == 0, 0.0, xp / (xp - s)), np.inf)
            alpha = al.min()
            xn = xp + alpha * (s - xp)
            drop = neg & (~(xn > 0) | (al == alpha))
            x[:] = 0.0
            x[P] = np.where(drop, 0.0, xn)
            left += int(drop.sum())
            P = [p for p, d in zip(P, drop) if not d]
            if not P:
                break
        w = gradient()
    J, n2 = E, 0.0
    for a in range(A):
        if x[a] != 0:
            J = J - x[a] * (f[a] + w[a])
            n2 = n2 + x[a] * x[a]
    if not np.isfinite(J):
        return nan, np.nan, np.nan, 2, solves, left
    return x, J, J - mu * n2, status, solves, left


def _nnls_chi2_task(H, valid, mu0, f, E, tol, nrec, base, chi2, rtol, max_evals=None, cap=None):
    """the search of `nnls_host(..., chi2=)` for one voxel in its chosen group (module docstring, steps 2 to 4).  base: the
    baseline `_nnls_task` result (x, J, J_data, status, ...) at mu0 -> (x, J_data, status, mu, ratio, evals); max_evals: the
    fits allowed, NNLS_CHI2_EVALS, and cap: that of the passive-set solves of a fit (tests lower them)"""
    A = len(f)
    max_evals = NNLS_CHI2_EVALS if max_evals is None else max_evals
    x0, _, Jd0, st0 = base[:4]
    if st0 != 0:
        return x0, Jd0, st0, mu0, 1.0, 0
    floor = 32.0 * float(nrec + A) * 2.0 ** -53 * E / rtol
    if not Jd0 > 0.0 or Jd0 < floor:
        return x0, Jd0, 4, mu0, 1.0, 0
    T = chi2 * Jd0
    if abs(Jd0 / T - 1.0) <= rtol:
        return x0, Jd0, 0, mu0, 1.0, 0
    if not T < E or not mu0 > 0.0:
        return x0, Jd0, 3, mu0, 1.0, 0
    out = (x0, Jd0, 3, mu0, 1.0)
    mu_lo, r_lo, mu_hi, r_hi, best = mu0, Jd0 / T - 1.0, 0.0, 0.0, Jd0
    bracket, side, evals = False, 0, 0
    while evals < max_evals:
        mu = mu_lo * NNLS_CHI2_FACTOR
        if bracket:
            mu = mu_lo * np.exp(r_lo / (r_lo - r_hi) * np.log(mu_hi / mu_lo))
        if not np.isfinite(mu):
            break
        evals += 1
        x, J, Jd, st = _nnls_task(H, valid, mu, f, E, tol, cap)[:4]
        if st != 0:
            break
        r = Jd / T - 1.0
        hit = abs(r) <= rtol
        if hit or (r < 0.0 and Jd > best):
            best = Jd
            out = (x, Jd, 3, mu, Jd / Jd0)
        if hit:
            out = out[:2] + (0,) + out[3:]
            break
        if r < 0.0:
            mu_lo, r_lo = mu, r
            if bracket:
                if side < 0:
                    r_hi *= 0.5
                side = -1
        else:
            mu_hi, r_hi = mu, r
            if bracket and side > 0:
                r_lo *= 0.5
            bracket, side = True, 1
    return out + (evals,)


def nnls_host(D, S, axis, *, reg=NNLS_REG, tol=NNLS_TOL, group=None, chi2=None, chi2_rtol=NNLS_CHI2_RTOL, _max_evals=None, _cap=None):
    """the method of `nnls` (module docstring) in NumPy float64 on host arrays: the documented definition -- the same active set on
    the Gram form, one (voxel, group) at a time.  Not a path of `nnls`, which never calls it, and any number of atoms.

    D `[nrec, *grid]`, S `[nrec, *shape]`, axis into `grid`; reg, tol, group, chi2, chi2_rtol as for `nnls`.  Returns an `NnlsResult`
    with `solves` and `left` filled (with chi2=: those of the baseline fit)."""
    D, S = np.asarray(D, dtype=np.complex128), np.asarray(S, dtype=np.complex128)
    if D.ndim < 2 or S.ndim < 1 or S.shape[0] != D.shape[0] or D.shape[0] < 1 or D.size == 0:
        raise ValueError(f"nnls_host: D [nrec, *grid], S [nrec, *shape]: got {D.shape}, {S.shape}")
    reg, tol = _nnls_reg_tol(reg, tol)
    chi2, chi2_rtol = _nnls_chi2(chi2, chi2_rtol, reg)
    nrec, shape = D.shape[0], S.shape[1:]
    axis, A, nouter, ninner, groups = _component_axis(axis, D.shape[1:])
    G = nouter * ninner
    Dg = np.moveaxis(D.reshape(nrec, nouter, A, ninner), 2, 1).reshape(nrec, A, G)
    s = S.reshape(nrec, -1)
    nmeas = s.shape[1]
    grp = _nnls_group(group, shape)
    with np.errstate(all="ignore"):
        H = np.einsum("tag,tbg->gab", Dg.real, Dg.real) + np.einsum("tag,tbg->gab", Dg.imag, Dg.imag)
        diag = np.einsum("gaa->ga", H)
        valid = np.isfinite(diag) & (diag > 0)
        mu = np.array([reg * (diag[g][valid[g]].sum() / valid[g].sum()) if valid[g].any() else 0.0 for g in range(G)])
        F = np.einsum("tag,tm->gma", Dg.real, s.real) + np.einsum("tag,tm->gma", Dg.imag, s.imag)
        E = (s.real ** 2 + s.imag ** 2).sum(axis=0)
    weights = np.full((A, nmeas), np.nan)
    chosen, status = np.full(nmeas, -1, dtype=np.int64), np.full(nmeas, 2, dtype=np.int32)
    residual = np.full(nmeas, np.nan)
    solves, left = np.zeros(nmeas, dtype=np.int64), np.zeros(nmeas, dtype=np.int64)
    ridge, ratio, evals = np.full(nmeas, np.nan), np.full(nmeas, np.nan), np.zeros(nmeas, dtype=np.int32)
    for m in range(nmeas):
        best, base = np.inf, None
        todo = range(G) if grp is None else ([int(grp.reshape(-1)[m])] if 0 <= grp.reshape(-1)[m] < G else [])
        for g in todo:
            with np.errstate(all="ignore"):
                task = _nnls_task(H[g], valid[g], mu[g], F[g, m], E[m], tol, _cap)
            x, J, Jd, st, ns, nl = task
            if st != 2 and J < best:
                best, base = J, task
                weights[:, m], chosen[m], status[m], solves[m], left[m] = x, g, st, ns, nl
                residual[m] = np.sqrt(max(Jd, 0.0))
        if chi2 is not None and base is not None:
            g = chosen[m]
            with np.errstate(all="ignore"):
                x, Jd, st, ridge[m], ratio[m], evals[m] = _nnls_chi2_task(H[g], valid[g], mu[g], F[g, m], E[m], tol, nrec, base, chi2,
                                                                         chi2_rtol, _max_evals, _cap)
            weights[:, m], status[m], residual[m] = x, st, np.sqrt(max(Jd, 0.0))
    more = {} if chi2 is None else dict(mu=ridge.reshape(shape), chi2=ratio.reshape(shape), evals=evals.reshape(shape))
    return NnlsResult(weights.reshape((A,) + shape), chosen.reshape(shape), residual.reshape(shape), status.reshape(shape), groups,
                      solves.reshape(shape), left.reshape(shape), **more)

"""Float wavenumbers: the planner and the execution of the shift-merge (epgpy/shift.py:367-449 `shiftmerge`).

A shift by a float wavenumber -- `S(1.5)`, a gradient `G(tau, [gx, gy, gz])`, the time accumulation `C(tau, R2)` -- moves
the rows of the state matrix to coordinates that fall on no integer lattice.  The reference quantises the shifted
coordinates on a grid (`kgrid`), lets the rows that share a grid cell merge (their values add up, their coordinate becomes the
average weighted by sum |state| over all voxels) and prunes the rows that are numerically empty in every voxel.

Which rows meet is a function of the coordinates alone: `MergePlan` reproduces shift.py:393-409 on the host and emits, for all
voxels at once, the table of the device's multi-source gather (epgx_state_merge).  What depends on the state -- the weights and
the pruning test -- are per-row reductions over all voxels that the device computes on the resident state
(epgx_state_row_stats); `MergePlan.finish` turns them into the new coordinates and the surviving rows (shift.py:420-444).

Such a shift cannot be planned ahead (the coordinates that the next shift quantises depend on the state), so it is a barrier
of the operator-by-operator path: `apply` launches what stands before it, runs  row stats -> merge -> row stats -> finish,
and goes on with the value-only operators on the new coordinate set (`FloatKSpace`).
"""
import numpy as np

from . import _lib, kspace

NAX = np.newaxis
VOXEL_HINT = "; the option voxel_coords=True (StateMatrix / simulate) runs it per voxel on the device"


class FloatKSpace(kspace.KSpace):
    """float coordinate set [R, kdim] of a state matrix after a shift-merge: symmetric about the centre row, shared by all
    voxels, ordered by grid cell (not necessarily by value).  Every row counts as populated: the pruning is numerical and has
    already happened.  Columns 0 .. 2 are wavenumbers, column 3 (if any) the accumulated time (statematrix.py:177-211)."""

    def __init__(self, coords, nz_f=None, nz_z=None, lead=()):
        pts = np.array(coords, dtype=np.float64)
        if lead:
            raise NotImplementedError("float coordinates that differ between voxels (shift-prune, shift.py:478-542)" + VOXEL_HINT)
        self.lead = ()
        self.points = pts.reshape(pts.shape[0], 1, pts.shape[-1])
        self.nz_f = self.nz_z = np.ones(len(pts), dtype=bool)
        assert len(self.points) % 2 == 1

    @classmethod
    def equilibrium(cls, kdim):
        return cls(np.zeros((1, kdim)))

    @classmethod
    def from_coords(cls, coords, kgrid=None, scale=1.0):
        """coordinates as `StateMatrix.coords` returns them, [1.., R, kdim] (checked: symmetric about the centre row; with a
        grid `kgrid` for the coordinates times `scale`: one row per grid cell, cells in lexicographic order)"""
        coords = np.asarray(coords, dtype=np.float64)
        if coords.ndim < 2 or coords.shape[-2] % 2 != 1:
            raise ValueError("coords: expected [..., 2n+1, kdim]")
        if any(d != 1 for d in coords.shape[:-2]):
            raise NotImplementedError("float coordinates that differ between voxels (shift-prune, shift.py:478-542)" + VOXEL_HINT)
        pts = coords.reshape(coords.shape[-2:])
        if not np.allclose(pts, -pts[::-1], rtol=1e-9, atol=1e-12 * max(1.0, float(np.abs(pts).max(initial=0.0)))):
            raise ValueError("coords: rows must be symmetric about the centre row")
        if kgrid is not None:
            cells = np.around(pts * scale / (kgrid * np.ones(pts.shape[-1]))).astype(np.int64)
            order = np.lexsort(cells.T[::-1])
            if not np.array_equal(order, np.arange(len(pts))) or (len(pts) > 1 and not np.all(np.any(np.diff(cells, axis=0) != 0, axis=1))):
                raise ValueError("coords: rows must fall into distinct grid cells, sorted lexicographically")
        return cls(pts)

    def with_kdim(self, kdim):
        if kdim == self.kdim:
            return self
        if kdim < self.kdim:
            raise RuntimeError("Cannot remove existing k-dimension")
        pts = self.points[:, 0, :]
        return FloatKSpace(np.concatenate([pts, np.zeros((len(pts), kdim - self.kdim))], axis=1))

    def with_lead(self, lead):
        if tuple(lead):
            raise NotImplementedError("float coordinates that differ between voxels (shift-prune, shift.py:478-542)" + VOXEL_HINT)
        return self

    def _like(self, nz_f, nz_z):
        return self

    def shifted(self, delta, nmax=None):
        raise NotImplementedError("a shift of float coordinates is a shift-merge (kmerge.apply), not a planned gather")

    def bmatrices(self, kvalue, shift=None):
        """as KSpace.bmatrices, over the wavenumber columns (the time coordinate does not diffuse: diffusion.py uses `sm.k`)"""
        if self.kdim <= 3:
            return super().bmatrices(kvalue, shift)
        return FloatKSpace(self.points[:, 0, :3]).bmatrices(kvalue, None if shift is None else np.asarray(shift).reshape(-1)[:3])


class VoxelKSpace(FloatKSpace):
    """float coordinates that differ between voxels, after a per-voxel shift (`shift_prune`): a device buffer [nvox][kdim][64]
    with the live stored rows per voxel (_lib.DeviceCoords) next to the state.  `nstate + 1` is the largest live count; a
    voxel's live rows are its stored orders 0 .. live - 1 in lexicographic order of their grid cells, the rest exact zeros.
    Row-local operators pass it on unchanged; whatever reads shared coordinates on the host (D, DFT / Imaging / System, the
    planned shifts) does not run on it."""

    def __init__(self, dev, grid, nstate):
        self.dev, self.grid, self._n = dev, tuple(int(d) for d in grid), int(nstate)
        self.lead = self.grid
        self.nz_f = self.nz_z = np.ones(2 * self._n + 1, dtype=bool)

    @classmethod
    def equilibrium(cls, kdim):
        """RESET: one row at the origin in every voxel -- shared coordinates again"""
        return FloatKSpace.equilibrium(kdim)

    @classmethod
    def from_coords(cls, ctx, coords, grid):
        """coordinates [*grid', 2n+1, kdim] as `StateMatrix.coords` exports them (grid' broadcasts to `grid`): per voxel the
        live rows centred and symmetric, zero rows at both ends"""
        coords = np.asarray(coords, dtype=np.float64)
        if coords.ndim < 2 or coords.shape[-2] % 2 != 1 or not 1 <= coords.shape[-1] <= 4:
            raise ValueError("coords: expected [..., 2n+1, kdim] with kdim 1 .. 4")
        n, kdim = (coords.shape[-2] - 1) // 2, coords.shape[-1]
        if n + 1 > _lib.PRUNE_K:
            raise NotImplementedError(f"per-voxel coordinates with more than {_lib.PRUNE_K} stored orders (kgrid / max_nstate / prune)")
        if not np.allclose(coords, -coords[..., ::-1, :], rtol=1e-9, atol=1e-12 * max(1.0, float(np.abs(coords).max(initial=0.0)))):
            raise ValueError("coords: rows must be symmetric about the centre row")
        lead = coords.shape[:-2]
        full = np.broadcast_to(coords.reshape(lead + (1,) * (len(grid) - len(lead)) + coords.shape[-2:]), tuple(grid) + coords.shape[-2:])
        half = full.reshape(-1, 2 * n + 1, kdim)[:, n:, :]
        used = np.any(half != 0, axis=-1)                       # (rows past the live ones are exact zeros)
        nlive = np.where(used.any(axis=1), n + 1 - np.argmax(used[:, ::-1], axis=1), 1).astype(np.int32)
        k = np.zeros((half.shape[0], kdim, _lib.PRUNE_K))
        k[:, :, : n + 1] = np.moveaxis(half, -1, -2)
        dev = _lib.DeviceCoords(ctx, half.shape[0], kdim)
        dev.upload(k, nlive)
        return cls(dev, grid, n)

    @property
    def points(self):
        raise NotImplementedError("per-voxel coordinates (voxel_coords) live on the device: D, DFT / Imaging / System and planned "
                                  "shifts read coordinates shared by all voxels and do not run on them")

    @property
    def kdim(self):
        return self.dev.kdim

    @property
    def nrow(self):
        return 2 * self._n + 1

    @property
    def coords(self):
        """[*grid, 2n+1, kdim]: downloaded and mirrored"""
        k, _ = self.dev.download()
        pos = np.moveaxis(k[:, :, : self._n + 1], -2, -1)
        return np.concatenate([0.0 - pos[:, :0:-1, :], pos], axis=1).reshape(self.grid + (self.nrow, self.kdim))

    def live(self):
        """live stored rows per voxel [*grid]"""
        return self.dev.download()[1].reshape(self.grid)

    def with_kdim(self, kdim):
        if kdim == self.kdim:
            return self
        if kdim < self.kdim:
            raise RuntimeError("Cannot remove existing k-dimension")
        return VoxelKSpace(self.dev.widen(kdim), self.grid, self._n)

    def with_lead(self, lead):
        if tuple(lead) != self.grid:
            raise NotImplementedError(f"widening the grid of a state matrix that holds per-voxel coordinates (voxel_coords): "
                                      f"{self.grid} -> {tuple(lead)}; give the state matrix its full shape before the first shift")
        return self

    def bmatrices(self, kvalue, shift=None):
        raise NotImplementedError("D (diffusion) on per-voxel coordinates (voxel_coords): the b-matrices are planned on the host "
                                  "from coordinates shared by all voxels")


def is_float(ks):
    """True for a coordinate set with float coordinates (after a float shift)"""
    return isinstance(ks, FloatKSpace)


def ktvalue(kvalue, tvalue, kdim):
    """what turns coordinates into wavenumbers (rad/m) and accumulated time (statematrix.py:202-211)"""
    if np.ndim(kvalue) == 0:
        coeff = [kvalue] * min(kdim, 3) + [tvalue] * (kdim == 4)
    else:
        coeff = list(kvalue)[:min(kdim, 3)] + [tvalue] * (kdim == 4)
    return np.asarray(coeff)


def unique_rows(values):
    """(unique rows in lexicographic order, index of every row among them): shift.py:461-475"""
    order = np.lexsort(values.T[::-1])
    ranked = values[order]
    mask = np.r_[True, np.any(np.diff(ranked, axis=0) != 0, axis=-1)]
    inverse = np.zeros_like(order)
    inverse[order] = np.cumsum(mask) - 1
    return ranked[mask], inverse


class MergePlan:
    """the state-independent half of `shiftmerge` for wavenumbers [R, kdim], a shift [kdim] and a grid (shift.py:393-409):
    the quantised coordinates, the three index lists and the table of epgx_state_merge.  `finish` is the other half."""

    def __init__(self, wavenums, shift, grid=1):
        wavenums = np.asarray(wavenums)
        shift = np.asarray(shift, dtype=np.float64).reshape(1, -1)
        if wavenums.ndim != 2 or wavenums.shape[0] % 2 != 1 or shift.shape[1] != wavenums.shape[1]:
            raise ValueError(f"MergePlan: wavenumbers {wavenums.shape}, shift {shift.shape}")
        grid = grid * np.ones(wavenums.shape[-1])
        n1 = len(wavenums)
        # (rounding prevents numerical noise from moving a coordinate over a cell boundary)
        self.kL = np.around(wavenums + 0 * shift, decimals=8)
        self.k1T = self.kL + shift
        self.k2T = self.kL - shift
        # quantise; qL is made symmetric, q2T is the mirror image of q1T
        qL = np.around(0.5 * (self.kL - self.kL[::-1]) / grid).astype(int)
        q1T = np.around(self.k1T / grid).astype(int)
        q2T = -q1T[::-1]
        self.q2, idx = unique_rows(np.concatenate([qL, q1T, q2T], axis=0))
        self.idxL, self.idx1T, self.idx2T = idx[:n1], idx[n1: 2 * n1], idx[2 * n1:]
        self.nrow_old, self.nrow = n1, len(self.q2)
        if self.nrow % 2 == 0:
            raise ValueError("Asymmetrical state matrix")
        self.offsets, self.sources = self._table()

    @property
    def nhalf(self):
        """stored orders of the destination"""
        return (self.nrow + 1) // 2

    def _table(self):
        """CSR table of epgx_state_merge over the stored orders j of the new matrix (row cn + j).  Column 2 goes by idxL, column
        0 by idx1T, column 1 is the mirror image of the new column 0 (shift.py:415-417); the sources of one destination in
        ascending row index of the old matrix -- the order in which np.add.at adds them.  Old row c0 + i is stored order i
        (components 0, 1, 2); old row c0 - i holds conj(B_i), conj(A_i), conj(Z_i)."""
        c0, cn, nh = (self.nrow_old - 1) // 2, (self.nrow - 1) // 2, self.nhalf
        CONJ, SH = _lib.GS_CONJ, _lib.MERGE_COMP_SHIFT
        rows_f = [[] for _ in range(self.nrow)]      # old rows whose column 0 lands in new row r2
        rows_z = [[] for _ in range(self.nrow)]
        for r in range(self.nrow_old):
            rows_f[self.idx1T[r]].append(r)
            rows_z[self.idxL[r]].append(r)

        def entry(r, above, below, conj_above):
            """source entry of old row r: component `above` of order r - c0, or `below` of order c0 - r (the mirror row holds
            the conjugate of the partner component); conj_above: the value is wanted conjugated"""
            if r >= c0:
                return (r - c0) | (above << SH) | (CONJ if conj_above else 0)
            return (c0 - r) | (below << SH) | (0 if conj_above else CONJ)

        lists = [[[entry(r, 0, 1, False) for r in rows_f[cn + j]] for j in range(nh)],
                 [[entry(r, 0, 1, True) for r in rows_f[cn - j]] for j in range(nh)],
                 [[entry(r, 2, 2, False) for r in rows_z[cn + j]] for j in range(nh)]]
        offsets, sources = np.zeros((3, nh + 1), dtype=np.int32), []
        for c in range(3):
            offsets[c, 0] = len(sources)
            for j in range(nh):
                sources.extend(lists[c][j])
                offsets[c, j + 1] = len(sources)
        return offsets, np.asarray(sources, dtype=np.int32)

    def finish(self, sums, maxabs, tol=1e-8, prune=True):
        """the state-dependent half (shift.py:420-444).  sums [3, n_old + 1]: sum over all voxels of |A_j|, |B_j|, |Z_j| of the
        OLD stored orders; maxabs [nhalf]: largest modulus of the NEW stored orders.  Returns (wavenumbers [R', kdim] of the
        surviving rows, the new stored orders they are: `keep`, ascending, keep[0] = 0)."""
        sums, maxabs = np.asarray(sums, dtype=np.float64), np.asarray(maxabs, dtype=np.float64)
        c0, cn = (self.nrow_old - 1) // 2, (self.nrow - 1) // 2
        if sums.shape != (3, c0 + 1) or maxabs.shape != (cn + 1,):
            raise ValueError(f"finish: sums {sums.shape}, maxabs {maxabs.shape} for {c0 + 1} -> {cn + 1} stored orders")
        # w[r, c] = sum over the voxels of |states[.., r, c]| (row -j: columns 0 and 1 swapped, the moduli of the conjugates)
        w = np.empty((self.nrow_old, 3))
        w[c0:] = sums.T
        w[:c0] = sums.T[:0:-1][:, [1, 0, 2]]
        wnorm = np.zeros(self.nrow)
        np.add.at(wnorm, self.idxL, w[:, 2])
        np.add.at(wnorm, self.idx1T, w[:, 0])
        np.add.at(wnorm, self.idx2T, w[:, 1])
        k2 = np.zeros(self.q2.shape, dtype=float)
        np.add.at(k2, (self.idxL, slice(None)), self.kL * w[:, 2:3])
        np.add.at(k2, (self.idx1T, slice(None)), self.k1T * w[:, 0:1])
        np.add.at(k2, (self.idx2T, slice(None)), self.k2T * w[:, 1:2])
        # rows that hold something in some voxel: isclose(x, 0, atol=tol) is |x| <= tol
        half = maxabs > tol
        nonzero = np.concatenate([half[:0:-1], half])
        wnorm[~nonzero] = 1.0
        k2 /= wnorm[:, NAX]
        if prune:
            nonzero[cn] = True      # (the centre row always stays)
            k2 = k2[nonzero]
            keep = np.flatnonzero(nonzero[cn:])
        else:
            keep = np.arange(cn + 1)
        if len(k2) % 2 == 0:
            raise ValueError("Asymmetrical state matrix")
        return k2, keep


def merges(shift_op, ks):
    """True if S-like `shift_op` takes the merge path on a state with coordinate set `ks` (get_shift_method, shift.py:213-254)"""
    return isinstance(ks, FloatKSpace) or shift_op._float_k()


def per_voxel(shift_op, ks):
    """True if a merging shift gives (or meets) coordinates that differ between voxels: the reference's 'shift-prune'
    (shift.py:247-249), and -- a deliberate deviation, DESIGN 4.14 -- every shift once the coordinates are per voxel"""
    return isinstance(ks, VoxelKSpace) or (merges(shift_op, ks) and np.sum(np.shape(shift_op.k)[:-1]) > 1)


def has_merge(ks, ops):
    from .shift import S
    return any(isinstance(op, S) and merges(op, ks) for op in ops)


def apply(sm, ops):
    """`ops` on `sm` where some shift is a shift-merge: the operators between two such shifts as one launch each
    (plan.apply_operators), the shifts through `shift_merge`"""
    from .plan import apply_operators
    from .shift import S

    if getattr(sm, "_eq", None) is not None:
        raise NotImplementedError("a float shift (shift-merge) on a state matrix with a general equilibrium")
    batch = []
    for op in ops:
        if isinstance(op, S) and merges(op, sm._kspace):
            if batch:
                sm = apply_operators(sm, batch)
                batch = []
            if sm.options.get("voxel_coords") and per_voxel(op, sm._kspace):
                sm = shift_prune(sm, op)
            else:
                sm = shift_merge(sm, op)
        else:
            batch.append(op)
    return apply_operators(sm, batch) if batch else sm


def shift_merge(sm, op):
    """S._apply, branch 'shift-merge' (shift.py:120-148), on the device-resident state of `sm`, in place"""
    if getattr(sm, "order1", None) or getattr(sm, "order2", None):
        raise NotImplementedError("derivative states (order1 / order2, Jacobian / Hessian) through a float shift (shift-merge)")
    k = op.k
    ks = sm._kspace
    if isinstance(k, int):          # onto float coordinates: [k, 0, ...] (shift.py:243-244)
        shift = np.array([[int(k)] + [0] * (ks.kdim - 1)])
    else:
        shift = np.asarray(k)
    if np.sum(np.shape(shift)[:-1]) > 1:
        raise NotImplementedError("a float wavenumber that varies along a grid axis (shift-prune, shift.py:247-249, :478-542): "
                                  "the coordinate sets would differ per voxel" + VOXEL_HINT)
    kgrid = sm.options.get("kgrid") or op.kgrid
    if kgrid is None:
        raise AttributeError("kgrid not set")
    prune = sm.options.get("prune") or op.prune
    tol = 1e-8 if prune in (True, False) else float(prune)
    prune = bool(prune)

    # coordinates of the matrix as it stands, with the columns of the shift (shift.py:122-127)
    kdim = shift.shape[-1]
    if ks is None:
        ks = kspace.KSpace.from_orders(sm.nstate, kdim)
    if ks.lead:
        raise NotImplementedError("a float shift of coordinates that differ between voxels (shift-prune, shift.py:478-542)" + VOXEL_HINT)
    if ks.kdim < kdim:
        ks = ks.with_kdim(kdim)
    elif kdim < ks.kdim:
        shift = np.pad(shift, [(0, 0)] * (shift.ndim - 1) + [(0, ks.kdim - kdim)])
    if ks.nstate != sm.nstate or sm.nstate + 1 > sm._state.K:
        raise NotImplementedError("a float shift of a state matrix that was truncated at its capacity")
    coords = ks.coords                                    # [R, kdim], int or float
    ktv = ktvalue(sm.kvalue, sm.tvalue, ks.kdim)
    plan = MergePlan(coords * ktv, np.asarray(shift).reshape(-1) * ktv, kgrid)

    ctx = sm._ctx
    sums, _ = _lib.state_row_stats(ctx, sm._state, sm.nstate + 1)
    K = next((K for K in _lib.SUPPORTED_K if K >= plan.nhalf), _lib.SUPPORTED_K[-1])     # (past 1024 stored orders the entry point refuses)
    dst = _lib.DeviceState(ctx, sm.size, K)
    _lib.state_merge(ctx, dst, sm._state, plan.nhalf, plan.offsets, plan.sources)
    _, maxabs = _lib.state_row_stats(ctx, dst, plan.nhalf)
    wavenums, keep = plan.finish(sums, maxabs, tol, prune)
    if len(keep) < plan.nhalf:
        compact(ctx, dst, keep, sm.shape)
    sm._state, sm._nstate = dst, len(keep) - 1
    sm._kspace = FloatKSpace(wavenums / ktv)
    return sm


def shift_prune(sm, op):
    """S._apply, branch 'shift-prune' (shift.py:120-148, :478-629), on the device-resident state of `sm`: every voxel sorts,
    merges, weighs, trims and prunes its own rows (epgx_state_prune_shift); two words come back per shift.  Every check of
    the arguments stands before the first change of `sm`; a voxel that overflows on the device raises after `sm` was broadcast
    to the shift's grid (its values unchanged)"""
    from . import common
    if getattr(sm, "order1", None) or getattr(sm, "order2", None):
        raise NotImplementedError("derivative states (order1 / order2, Jacobian / Hessian) through a per-voxel float shift (shift-prune)")
    ks = sm._kspace
    if isinstance(op.k, int):       # onto existing coordinates: [k, 0, ...] (shift.py:243-244)
        shift = np.zeros((1, ks.kdim if ks is not None else 1))
        shift[0, 0] = op.k
    else:
        shift = np.asarray(op.k, dtype=np.float64)
    kgrid = sm.options.get("kgrid") or op.kgrid
    if kgrid is None:
        raise AttributeError("kgrid not set")
    if np.ndim(kgrid) > 1:
        raise NotImplementedError("a different kgrid per voxel: the grid is a scalar or one value per coordinate column")
    nmax = sm.options.get("max_nstate") or op.nmax or None
    prune = sm.options.get("prune") or op.prune
    tol = 1e-8 if prune in (True, False) else float(prune)
    prune = bool(prune)

    grid = tuple(common.broadcast_shapes(sm.shape, shift.shape[:-1], append=True))
    if len(grid) > _lib.PRUNE_MAX_DIMS:
        raise NotImplementedError(f"a per-voxel shift on a grid of more than {_lib.PRUNE_MAX_DIMS} axes")
    # every check that can raise stands before the first change of `sm`
    if isinstance(ks, VoxelKSpace) and (grid != sm.shape or ks.grid != sm.shape):
        raise NotImplementedError(f"widening the grid of a state matrix that holds per-voxel coordinates (voxel_coords): {ks.grid} -> "
                                  f"{grid}; give the state matrix its full shape before the first per-voxel shift")
    if sm.nstate + 1 > _lib.PRUNE_K or (ks is not None and ks.nstate != sm.nstate):
        raise NotImplementedError(f"a per-voxel float shift (shift-prune) of more than {_lib.PRUNE_K} stored orders: a coarser "
                                  "`kgrid`, a `max_nstate` or a larger `prune` tolerance keeps the state matrix under the limit")
    if ks is not None and not isinstance(ks, VoxelKSpace) and ks.lead:
        raise NotImplementedError("a per-voxel float shift of integer coordinates that differ along a leading grid axis")
    if grid != sm.shape:
        if len(grid) > sm.ndim:
            sm.expand(len(grid))
        sm._broadcast_to(grid)
    kdim = max(shift.shape[-1], ks.kdim if ks is not None else 1)
    if shift.shape[-1] < kdim:
        shift = np.pad(shift, [(0, 0)] * (shift.ndim - 1) + [(0, kdim - shift.shape[-1])])
    ctx = sm._ctx
    if isinstance(ks, VoxelKSpace):
        csrc = ks.with_kdim(kdim).dev
    else:       # coordinates shared by all voxels: one upload, repeated on the device
        if ks is None:
            ks = kspace.KSpace.from_orders(sm.nstate, kdim)
        half = np.asarray(ks.with_kdim(kdim).coords, dtype=np.float64)[ks.centre:]
        k = np.zeros((1, kdim, _lib.PRUNE_K))
        k[0, :, : len(half)] = half.T
        csrc = _lib.DeviceCoords(ctx, sm.size, kdim)
        csrc.upload(k, [len(half)])
    src = sm._state if sm._state.K == _lib.PRUNE_K else sm._state.copy(_lib.PRUNE_K)

    ktv = ktvalue(sm.kvalue, sm.tvalue, kdim).astype(np.float64)
    kshape = shift.shape[:-1]
    strides = [int(np.prod(kshape[d + 1:], dtype=np.int64)) if kshape[d] > 1 else 0 for d in range(len(kshape))]
    sstride = strides + [0] * (len(grid) - len(kshape))
    dst, cdst = _lib.DeviceState(ctx, sm.size, _lib.PRUNE_K), _lib.DeviceCoords(ctx, sm.size, kdim)
    live = _lib.state_prune_shift(ctx, dst, cdst, src, csrc, shift.reshape(-1, kdim) * ktv, grid, sstride, ktv,
                                  kgrid * np.ones(kdim), nmax, prune, tol)
    sm._state, sm._nstate = dst, live - 1
    sm._kspace = VoxelKSpace(cdst, grid, live - 1)
    return sm


def compact(ctx, state, keep, grid):
    """new stored order j <- stored order keep[j], the rest zero: the pruned rows leave through the single-source gather
    (EPGX_OP_GS), in place"""
    from .plan import Encoder

    enc = Encoder(grid)
    tab = np.tile(np.asarray(keep, dtype=np.int32), (3, 1))

    def build(K):
        full = np.full((3, K), _lib.GS_ZERO, dtype=np.int32)
        full[:, : tab.shape[1]] = tab
        return full.reshape(-1).view(np.float64)[None, :]

    enc.add_deferred(_lib.OP_GS, build)
    plan = enc.device_plan(ctx, state.K)
    _lib.run(ctx, plan, 0, plan.n_ops, 0, plan.nvox, state, state, state.K, None, 0, 0)

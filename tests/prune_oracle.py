"""NumPy restatement of the per-voxel float shift ('shift-prune'), one voxel at a time, in the full representation.

Written from the description of the semantics, not from the reference's code: a voxel is a list of rows
(F, col1, Z) with a wavenumber each, symmetric about the centre row.  `shift_voxel` returns a map  cell -> (F, col1, Z, k)
of the rows that survive; `layout` lays maps out as the state matrix exports them ([*grid, 2n+1, .], live rows centred in
lexicographic order of their cells, exact zeros at both ends).
"""
import numpy as np


def rnd(x):
    """round half away from zero, as the reference's own `round` followed by astype(int)"""
    return np.trunc(x - 0.5 + (x > 0))


def modulus(z):
    return np.sqrt(z.real * z.real + z.imag * z.imag)


def energy(z):
    return z.real * z.real + z.imag * z.imag


def shift_voxel(states, k, shift, grid, nmax=None, prune=True, tol=1e-8, details=None):
    """states [R, 3] complex, k [R, kdim] wavenumbers (already times ktvalue), shift [kdim], grid [kdim] or scalar.
    Returns {cell (tuple of int): (F, col1, Z, k [kdim])}.  details: a dict that receives what a generator wants to assert on"""
    states = np.asarray(states, dtype=np.complex128)
    k = np.asarray(k, dtype=np.float64)
    R, kdim = k.shape
    shift = np.asarray(shift, dtype=np.float64).reshape(kdim)
    grid = grid * np.ones(kdim)
    xL, x1T = 0.5 * (k - k[::-1]) / grid, (k + shift) / grid
    qL, q1T = rnd(xL), rnd(x1T)
    q2T = -q1T[::-1]
    key = lambda q: tuple(int(v) for v in q)
    F, Z, W, K, nsrc = {}, {}, {}, {}, {}

    def touch(cell):
        if cell not in W:
            F[cell], Z[cell], W[cell], K[cell], nsrc[cell] = 0j, 0j, 0.0, np.zeros(kdim), 0

    # Z stays, F moves by +s, column 1 mirrors it: sources in ascending row, from +0; weights and coordinates over all L,
    # then all 1T, then all 2T candidates
    for r in range(R):
        cell = key(qL[r])
        touch(cell)
        Z[cell] = Z[cell] + states[r, 2]
        w = modulus(states[r, 2])
        W[cell], K[cell], nsrc[cell] = W[cell] + w, K[cell] + k[r] * w, nsrc[cell] + 1
    for r in range(R):
        cell = key(q1T[r])
        touch(cell)
        F[cell] = F[cell] + states[r, 0]
        w = modulus(states[r, 0])
        W[cell], K[cell], nsrc[cell] = W[cell] + w, K[cell] + (k[r] + shift) * w, nsrc[cell] + 1
    for r in range(R):
        cell = key(q2T[r])
        touch(cell)
        w = modulus(states[r, 1])
        W[cell], K[cell], nsrc[cell] = W[cell] + w, K[cell] + (k[r] - shift) * w, nsrc[cell] + 1

    cells = sorted(W)
    zero = (0,) * kdim
    rows = {}
    for cell in cells:
        neg = tuple(-v for v in cell)
        col1 = np.conj(F.get(neg, 0j))
        rows[cell] = (F[cell], col1, Z[cell], K[cell] / (W[cell] + (W[cell] < 1e-12)))
    mag = {cell: (energy(rows[cell][0]) + energy(rows[cell][1])) + energy(rows[cell][2]) for cell in cells}
    positive = [cell for cell in cells if cell > zero]
    kept = set(cells)
    trimmed = False
    if nmax is not None and len(positive) > nmax:
        # the nmax positive rows of largest energy (ties: the later row), their mirrors and the centre row
        order = sorted(range(len(positive)), key=lambda i: (mag[positive[i]], i))
        top = {positive[i] for i in order[len(positive) - nmax:]}
        kept = {zero} | top | {tuple(-v for v in cell) for cell in top}
        trimmed = True
        if details is not None and nmax > 0:
            e = sorted(mag[c] for c in positive)
            details.setdefault("trim_cut", []).append((e[len(positive) - nmax - 1], e[len(positive) - nmax]))
    if prune:
        kept = {cell for cell in kept if cell == zero or np.sqrt(mag[cell]) > tol}
    if details is not None:
        details.setdefault("margin", []).extend(np.abs(np.concatenate([xL, x1T]) % 1.0 - 0.5).reshape(-1))
        details.setdefault("norms", []).extend(float(np.sqrt(mag[c])) for c in cells if c != zero)
        details.setdefault("merged_distinct", []).append(any(nsrc[c] > 1 for c in cells))
        details.setdefault("sources", {}).update({c: nsrc[c] for c in cells})
        details.setdefault("pruned", []).append(len(cells) - len(kept) if not trimmed else 0)
        details.setdefault("trimmed", []).append(trimmed)
    return {cell: rows[cell] for cell in cells if cell in kept}


def live_rows(states, coords):
    """the live rows of one exported voxel ([2n+1, 3], [2n+1, kdim]): what is left after dropping the zero rows at both ends"""
    n = (states.shape[0] - 1) // 2
    used = np.any(states != 0, axis=-1) | np.any(coords != 0, axis=-1)
    used = used | used[::-1]
    m = max([abs(r - n) for r in range(2 * n + 1) if used[r]], default=0)
    return states[n - m: n + m + 1], coords[n - m: n + m + 1]


def shift(states, coords, shifts, ktvalue, grid, nmax=None, prune=True, tol=1e-8, details=None):
    """all voxels: states [*vgrid, 2n+1, 3], coords [*vgrid, 2n+1, kdim] (as exported), shifts [*vgrid, kdim] (coordinates'
    units times ktvalue already applied by the caller: wavenumbers).  Returns the list of per-voxel maps, C order"""
    vgrid = states.shape[:-2]
    states, coords = states.reshape((-1,) + states.shape[-2:]), coords.reshape((-1,) + coords.shape[-2:])
    shifts = np.broadcast_to(shifts, vgrid + shifts.shape[-1:]).reshape(-1, shifts.shape[-1])
    maps = []
    for v in range(states.shape[0]):
        st, co = live_rows(states[v], coords[v])
        maps.append(shift_voxel(st, co * ktvalue, shifts[v], grid, nmax, prune, tol, details))
    return maps


def layout(maps, vgrid, ktvalue):
    """the maps of all voxels as (states [*vgrid, 2n+1, 3], coords [*vgrid, 2n+1, kdim]): n + 1 the largest number of stored
    rows, every voxel's rows centred in lexicographic order of the cells, coordinates = wavenumbers / ktvalue"""
    kdim = len(next(iter(maps[0])))
    n = max((len(m) - 1) // 2 for m in maps)
    states = np.zeros((len(maps), 2 * n + 1, 3), dtype=np.complex128)
    coords = np.zeros((len(maps), 2 * n + 1, kdim))
    for v, m in enumerate(maps):
        cells = sorted(m)
        assert len(cells) % 2 == 1
        at = n - (len(cells) - 1) // 2
        for i, cell in enumerate(cells):
            states[v, at + i] = m[cell][:3]
            coords[v, at + i] = m[cell][3] / ktvalue
    return states.reshape(tuple(vgrid) + states.shape[1:]), coords.reshape(tuple(vgrid) + coords.shape[1:])


def rows_by_cell(states, k, grid):
    """one exported voxel ([2n+1, 3], wavenumbers [2n+1, kdim]) as {cell: (states [3], k [kdim])}, the all-zero rows (padding)
    left out; the centre row always stays"""
    grid = grid * np.ones(k.shape[-1])
    used = np.any(states != 0, axis=-1) | np.any(k != 0, axis=-1)
    used[(len(used) - 1) // 2] = True
    out = {}
    for st, kk in zip(states[used], k[used]):
        cell = tuple(int(c) for c in rnd(kk / grid))
        assert cell not in out, f"two rows in cell {cell}"
        out[cell] = (st, kk)
    return out

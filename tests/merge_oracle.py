"""NumPy restatement of the float-wavenumber shift (shift-merge; Gao et al., Magn Reson Med 2021; 86:551-560) on the FULL
state matrix [*grid, R, 3] -- rows -n .. n, columns F+, F-, Z -- next to wavenumbers [R, kdim] shared by all voxels.

Own code: the tests compare it with recorded results of the reference (tests/golden/g22_merge.npz) and the device path
with it.  Also here: the half representation the device stores ([nvox][3][K], stored order j = row n + j), a NumPy
application of the multi-source gather table, and the per-row reductions the device computes.
"""
import numpy as np

GS_CONJ, COMP_SHIFT, ORDER_MASK = 1 << 30, 16, 0xffff


def lex_unique(rows):
    """(unique rows, lexicographically sorted -- first column most significant; index of every input row among them)"""
    order = np.lexsort(rows.T[::-1])
    ranked = rows[order]
    first = np.ones(len(rows), dtype=bool)
    first[1:] = np.any(ranked[1:] != ranked[:-1], axis=1)
    inverse = np.empty(len(rows), dtype=np.int64)
    inverse[order] = np.cumsum(first) - 1
    return ranked[first], inverse


def shiftmerge(states, wavenums, shift, grid=1, prune=True, tol=1e-8, details=False):
    """states [*grid, R, 3], wavenums [R, kdim], shift [kdim] -> (new states, new wavenumbers).
    details=True: also the unpruned states and the mask of the rows that survive"""
    sm = np.asarray(states, dtype=np.complex128)
    k = np.asarray(wavenums, dtype=np.float64).reshape(-1, np.shape(wavenums)[-1])
    d = np.asarray(shift, dtype=np.float64).reshape(1, -1)
    cell = grid * np.ones(k.shape[1])
    n1 = k.shape[0]
    lead = tuple(range(sm.ndim - 2))

    k_z = np.around(k + 0 * d, decimals=8)              # Z stays, F+ moves by +d, F- by -d
    k_p, k_m = k_z + d, k_z - d
    q_z = np.around(0.5 * (k_z - k_z[::-1]) / cell).astype(int)
    q_p = np.around(k_p / cell).astype(int)
    q_m = -q_p[::-1]
    q_new, where = lex_unique(np.concatenate([q_z, q_p, q_m]))
    i_z, i_p, i_m = where[:n1], where[n1:2 * n1], where[2 * n1:]
    n2 = len(q_new)

    out = np.zeros(sm.shape[:-2] + (n2, 3), dtype=np.complex128)
    np.add.at(out, (..., i_z, 2), sm[..., 2])
    np.add.at(out, (..., i_p, 0), sm[..., 0])
    out[..., 1] = out[..., ::-1, 0].conj()

    w = np.sum(np.abs(sm), axis=lead)                   # [R, 3]
    total = np.zeros(n2)
    k_new = np.zeros((n2, k.shape[1]))
    for idx, col, kk in ((i_z, 2, k_z), (i_p, 0, k_p), (i_m, 1, k_m)):
        np.add.at(total, idx, w[:, col])
        np.add.at(k_new, (idx, slice(None)), kk * w[:, col:col + 1])
    alive = np.max(np.abs(out), axis=lead + (out.ndim - 1,)) > tol      # some voxel holds more than tol in this row
    total[~alive] = 1.0
    k_new /= total[:, None]
    full = out
    if prune:
        alive = alive.copy()
        alive[(n2 - 1) // 2] = True
        out, k_new = out[..., alive, :], k_new[alive]
    if details:
        return out, k_new, full, alive
    return out, k_new


# ------------------------------------------------------------------------------------------------ half representation
def fold(states, K):
    """[*grid, 2n+1, 3] -> [nvox, 3, K]: stored order j = row n + j, components (F_j, conj(F_-j), Z_j)"""
    n = (states.shape[-2] - 1) // 2
    half = np.zeros((int(np.prod(states.shape[:-2], dtype=np.int64)), 3, K), dtype=np.complex128)
    half[:, :, :n + 1] = np.moveaxis(states[..., n:, :].reshape(-1, n + 1, 3), -1, -2)
    return half


def unfold(half, grid, n):
    """[nvox, 3, K] -> [*grid, 2n+1, 3]: row -j is the conjugate of stored order j with the F columns swapped"""
    pos = np.moveaxis(half[:, :, :n + 1], -2, -1)
    neg = pos[:, :0:-1, :][..., [1, 0, 2]].conj()
    return np.concatenate([neg, pos], axis=-2).reshape(tuple(grid) + (2 * n + 1, 3))


def apply_table(half, offsets, sources, Kd):
    """the multi-source gather in NumPy: dst[v][c][j] = the listed sources of src[v], added in the order listed from +0;
    a source entry is order | component << 16 | GS_CONJ"""
    offsets, sources = np.asarray(offsets), np.asarray(sources)
    dst = np.zeros((half.shape[0], 3, Kd), dtype=np.complex128)
    for c in range(3):
        for j in range(offsets.shape[1] - 1):
            for s in range(offsets[c, j], offsets[c, j + 1]):
                ent = int(sources[s])
                val = half[:, (ent >> COMP_SHIFT) & 3, ent & ORDER_MASK]
                dst[:, c, j] = dst[:, c, j] + (val.conj() if ent & GS_CONJ else val)
    return dst


def modulus(z):
    """|z| as the device evaluates it: sqrt(re re + im im), every operation rounded on its own"""
    return np.sqrt(z.real * z.real + z.imag * z.imag)


def row_stats(half, nrow):
    """(sums [3, nrow], maxabs [nrow]) over all voxels of the stored orders j < nrow"""
    mod = modulus(half[:, :, :nrow])
    return mod.sum(axis=0), mod.max(axis=(0, 1))

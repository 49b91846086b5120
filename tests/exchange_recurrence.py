"""A small NumPy EPG-X recurrence (full state matrix, rows k = -n .. n) for T / E / S / X / SPOILER / ADC sequences: the
checker of the exchange tests and of tools/bench_exchange.py.  It follows the reference's operator algebra
(exchange.py:89-120 for X) on the host, with the operators' own tables."""
import numpy as np

from epgpy_amd import epg


def _bcast(arr, lead, grid):
    """[*lead, ...tail] operator array -> [*grid, ...tail] (the reference's trailing-axes broadcasting)"""
    arr = np.asarray(arr)
    tail = arr.shape[len(lead):]
    arr = arr.reshape(tuple(lead) + (1,) * (len(grid) - len(lead)) + tail)
    return np.broadcast_to(arr, tuple(grid) + tail)


def recurrence(seq, grid, density, nmax):
    """full state matrix [*grid, 2 nmax + 1, 3] (rows k = -nmax .. nmax), from equilibrium, no truncation within nmax"""
    grid = tuple(grid)
    dens = np.broadcast_to(np.asarray(density, dtype=np.float64).reshape(
        np.shape(density) + (1,) * (len(grid) - np.ndim(density))), grid)
    st = np.zeros(grid + (2 * nmax + 1, 3), dtype=np.complex128)
    st[..., nmax, 2] = dens
    out = []
    for op in seq:
        if isinstance(op, epg.X):
            ax, n = op.axis, op.ncomp
            mT = np.moveaxis(op.mat[..., 0], (ax, ax + 1), (-2, -1))          # [*lead, N, N], lead has 1 at ax
            mL = np.moveaxis(op.mat[..., 2], (ax, ax + 1), (-2, -1))
            lead = mT.shape[:-2]
            mT = _bcast(np.expand_dims(mT, ax), lead[:ax] + (1,) + lead[ax:], grid)   # [*grid(1 at ax), N, N]
            mL = _bcast(np.expand_dims(mL, ax), lead[:ax] + (1,) + lead[ax:], grid)
            sub = st.copy()
            sub[..., nmax, 2] -= dens
            sub = np.moveaxis(sub, ax, -1)                   # [..., rows, 3, N]
            mTm = np.moveaxis(mT, ax, -3)[..., 0, :, :]      # grid without ax, N, N
            mLm = np.moveaxis(mL, ax, -3)[..., 0, :, :]
            new = np.empty_like(sub)
            new[..., 0, :] = np.einsum("...ij,...rj->...ri", mTm, sub[..., 0, :])
            new[..., 1, :] = np.einsum("...ij,...rj->...ri", mTm.conj(), sub[..., 1, :])
            new[..., 2, :] = np.einsum("...ij,...rj->...ri", mLm.real, sub[..., 2, :])
            st = np.moveaxis(new, -1, ax)
            st[..., nmax, 2] += dens
        elif isinstance(op, epg.T):
            mat = _bcast(op.mat, op.mat.shape[:-2], grid)
            st = np.einsum("...ij,...rj->...ri", mat, st)
        elif isinstance(op, epg.E):
            arr = _bcast(op.arr, op.arr.shape[:-1], grid)
            st = st * arr[..., None, :]
            if op.arr0 is not None:
                st[..., nmax, 2] += _bcast(op.arr0, op.arr0.shape[:-1], grid)[..., 2] * dens
        elif isinstance(op, epg.S):
            k = int(op.k)
            new = np.zeros_like(st)
            rows = st.shape[-2]
            if k > 0:
                new[..., k:, 0] = st[..., : rows - k, 0]
                new[..., : rows - k, 1] = st[..., k:, 1]
            else:
                new[..., : rows + k, 0] = st[..., -k:, 0]
                new[..., -k:, 1] = st[..., : rows + k, 1]
            new[..., 2] = st[..., 2]
            st = new
        elif op is epg.SPOILER:
            st = st.copy()
            st[..., :2] = 0
        elif isinstance(op, epg.Probe):
            out.append(st[..., nmax, 0].copy())
        else:
            raise TypeError(op)
    return np.stack(out)

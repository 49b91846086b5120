"""The plain signal in extended precision: a thin layer over tests/jacobian_recurrence.py (the same operators' closed forms,
no variables), the checker of tests/test_gpu_signal_paths.py.

    signal_recurrence(ops)                     -> records [record, *grid]                        (np.clongdouble)
    signal_recurrence(ops, return_state=True)  -> (records, state [*grid, 2 n + 1, 3])           rows k = -n .. n, the
                                                                                                  reference's growing n

Operators (oracle tuples, tests/sequences.py): T, E, P, R, S(n) for any integer n, 1-D D, ADC F0 / Z0 with a phase, SPOILER,
RESET, PD with and without reset, a start state `init`.  A COMBINED operator -- ("C", [factor tuples]): a product such as
E . T . E that the device runs as ONE general-matrix record (EPGX_OP_MAT) -- is its factors applied one after another.

Out of scope, each with a suite of its own or a float64 oracle only: n-D and gather shifts and 3-D diffusion
(tests/test_gpu_nd_paths.py against tests/nd_recurrence.py), DFT probes (tests/test_gpu_imaging.py), float shifts
(tests/test_gpu_merge.py), epg.X (tests/test_gpu_exchange_paths.py), RFPulse (tests/test_gpu_rfpulse.py), the tiled path
(tests/test_gpu_tiled.py)."""
import numpy as np

from oracle import epg_numpy as onp
from tests.jacobian_recurrence import jacobian_recurrence, grid_of


def factors(ops):
    """combined operators replaced by their factors, in the order they act"""
    out = []
    for op in ops:
        out += list(op[1]) if op[0] == "C" else [op]
    return out


def signal_grid(ops):
    return grid_of(factors(ops))


def signal_recurrence(ops, *, shape=None, max_nstate=None, init=None, kvalue=1.0, dtype=np.clongdouble, return_state=False):
    flat = factors(ops)
    grid = tuple(shape) if shape is not None else grid_of(flat)
    res = jacobian_recurrence(flat, [], probe=None, shape=grid, max_nstate=max_nstate, init=init, kvalue=kvalue, dtype=dtype,
                              return_state=return_state)
    return (res[0][..., 0], res[1]) if return_state else res[..., 0]


def oracle_signal(ops, *, shape=None, max_nstate=None, init=None, kvalue=1.0, return_state=False):
    """the float64 NumPy oracle on the same tuples (combined operators as their factors).  oracle.simulate has neither R nor D:
    a sequence with one of them runs the recurrence itself in float64, as tests/test_jacobian_recurrence_host.py does for D"""
    flat = factors(ops)
    grid = tuple(shape) if shape is not None else grid_of(flat)
    if any(op[0] in ("R", "D") for op in flat):
        return signal_recurrence(ops, shape=grid, max_nstate=max_nstate, init=init, kvalue=kvalue, dtype=np.complex128,
                                 return_state=return_state)
    sig, state = onp.simulate(flat, shape=grid, max_nstate=max_nstate, init=init, return_states=True)
    return (sig, state) if return_state else sig


def half_of(state):
    """[*grid, 2 n + 1, 3] -> the device's half layout [*grid, 3, n + 1]: F_k, conj(F_-k), Z_k for k = 0 .. n"""
    n = (state.shape[-2] - 1) // 2
    return np.moveaxis(np.asarray(state)[..., n:, :], -1, -2)


def record_errors(got, want):
    """[err_r]: max over voxels |got[r] - want[r]| / max over voxels |want[r]|; a record whose reference is identically zero
    must be exactly zero (inf otherwise)"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (got.shape, want.shape)
    errs = []
    for r in range(want.shape[0]):
        scale = float(np.max(np.abs(want[r]))) if want[r].size else 0.0
        diff = float(np.max(np.abs(got[r].astype(np.clongdouble) - want[r]))) if want[r].size else 0.0
        errs.append((0.0 if diff == 0.0 else np.inf) if scale == 0.0 else diff / scale)
    return errs


def order_errors(got_half, want_state):
    """[err_k], k = 0 .. K - 1 of the buffer got_half [*grid, 3, K] against want_state [*grid, 2 n + 1, 3]: the scale of
    order k is the maximum over voxels and the three components of |want[..., k, :]|; an order whose reference is identically
    zero -- every order above n among them -- must be exactly zero (inf otherwise)"""
    got = np.asarray(got_half)
    want = half_of(want_state)
    n1, K = want.shape[-1], got.shape[-1]
    assert got.shape[:-1] == want.shape[:-1] and K >= n1, (got.shape, want.shape)
    errs = []
    for k in range(K):
        if k >= n1:
            errs.append(0.0 if not got[..., k].any() else np.inf)
            continue
        scale = float(np.max(np.abs(want[..., k])))
        diff = float(np.max(np.abs(got[..., k].astype(np.clongdouble) - want[..., k])))
        errs.append((0.0 if diff == 0.0 else np.inf) if scale == 0.0 else diff / scale)
    return errs

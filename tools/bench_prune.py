"""Time the per-voxel float shift (shift-prune) on a grid, per shift.

    python tools/bench_prune.py [side] [repeats]      # defaults 512 (a 512 x 512 grid), 20

For 16 and 64 stored orders and kdim 1 and 4: epgx_state_prune_shift on a populated state (every voxel `n` live rows on an
integer lattice with a small per-voxel offset, a per-voxel shift that stays inside the cells, so `n` rows come out), one
warm-up call, then best and mean of `repeats`.  The host clock stands around the whole call: the upload of the shift table,
both kernels, the two words that come back and the synchronisations.  Against it the byte model (48 + 8 kdim)(K_src + K_dst)
per voxel (K = 64 rows stored either side) at the 6.29 TB/s copy rate, and -- measured in the same process -- the
shared-coordinate float shift of DESIGN 4.9 (S(1.37) through op(sm): row stats, merge, row stats, finish) on a grid of the
same size and about the same number of stored orders.
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from epgpy_amd import epg, _lib  # noqa: E402

side = int(sys.argv[1]) if len(sys.argv) > 1 else 512
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
nvox, K = side * side, _lib.PRUNE_K
ctx = _lib.get_context()


def timed(fn):
    fn()
    ctx.synchronize()
    best, total = 1e9, 0.0
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ctx.synchronize()
        dt = time.perf_counter() - t0
        best, total = min(best, dt), total + dt
    return best * 1e3, total / reps * 1e3


def populated(n, kdim, seed=0):
    """device state and coordinates of `nvox` voxels with n live rows each, and a shift per voxel"""
    rng = np.random.default_rng(seed)
    tile = 4096                                        # (distinct voxels; repeated to fill the grid)
    half = np.zeros((tile, 3, K), dtype=np.complex128)
    half[:, :, :n] = rng.normal(size=(tile, 3, n)) + 1j * rng.normal(size=(tile, 3, n))
    half[:, 2, 0] = half[:, 2, 0].real
    half[:, 1, 0] = half[:, 0, 0].conj()
    k = np.zeros((tile, kdim, K))
    k[:, 0, :n] = np.arange(n)
    k[:, :, 1:n] += rng.uniform(-0.1, 0.1, size=(tile, kdim, n - 1))
    shifts = rng.uniform(0.05, 0.3, size=(tile, kdim))
    times = -(-nvox // tile)
    state, coords = _lib.DeviceState(ctx, nvox, K), _lib.DeviceCoords(ctx, nvox, kdim)
    state.upload(np.tile(half, (times, 1, 1))[:nvox], np.ones(nvox))
    coords.upload(np.tile(k, (times, 1, 1))[:nvox], np.full(nvox, n, np.int32))
    return state, coords, np.tile(shifts, (times, 1))[:nvox]


for n in (16, 64):
    for kdim in (1, 4):
        src, csrc, shifts = populated(n, kdim)
        dst, cdst = _lib.DeviceState(ctx, nvox, K), _lib.DeviceCoords(ctx, nvox, kdim)
        live = []
        best, mean = timed(lambda: live.append(_lib.state_prune_shift(ctx, dst, cdst, src, csrc, shifts, [nvox], [1], np.ones(kdim),
                                                                      np.ones(kdim), None, True, 1e-8)))
        model = (48 + 8 * kdim) * 2 * K * nvox / 6.29e12 * 1e3
        print(f"prune shift {side}x{side} stored orders {n} -> {live[-1]} kdim={kdim}: {best:.3f} ms best, {mean:.3f} ms mean of {reps}; "
              f"byte model {model:.3f} ms -> {model / best:.1%} of the copy rate", flush=True)
        del src, csrc, dst, cdst

for n in (16, 64):
    sm = epg.StateMatrix(shape=(side, side), kgrid=1.0)
    for op in [epg.T(90, 90)] + [epg.S(1.37), epg.T(np.linspace(100, 170, side), 0)] * (2 * n):
        sm = op(sm, inplace=True)
        if sm.nstate + 1 >= n:
            break
    shift, times = epg.S(1.37), []
    for _ in range(1 + min(reps, 5)):                  # (the matrix grows with every shift: a few calls, the first a warm-up)
        t0 = time.perf_counter()
        sm = shift(sm, inplace=True)
        ctx.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    print(f"shared-coordinate float shift {side}x{side} stored orders -> {sm.nstate + 1}: {min(times[1:]):.3f} ms best, "
          f"{sum(times[1:]) / len(times[1:]):.3f} ms mean of {len(times) - 1} (op(sm): row stats, merge, row stats, finish)", flush=True)

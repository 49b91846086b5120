"""Time the two kernels of the float-wavenumber shift and one whole float shift.

    python tools/bench_merge.py [nvox] [K] [repeats]      # defaults 262144, 64, 20

row stats: epgx_state_row_stats per call (kernels + the 4 K doubles that come back), against 48 K bytes per voxel at the copy
rate.  merge: epgx_state_merge with a one-source-per-order table (the table upload included).  shift: S(1.37) on a populated
state matrix through op(sm) -- row stats, merge, row stats, finish.  Host clock around calls that end in a synchronisation.
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from epgpy_amd import epg, _lib  # noqa: E402

nvox = int(sys.argv[1]) if len(sys.argv) > 1 else 262144
K = int(sys.argv[2]) if len(sys.argv) > 2 else 64
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 20
ctx = _lib.get_context()
src, dst = _lib.DeviceState(ctx, nvox, K), _lib.DeviceState(ctx, nvox, K)
offsets = np.tile(np.arange(K + 1, dtype=np.int32), (3, 1)) + (np.arange(3, dtype=np.int32) * K)[:, None]
sources = np.concatenate([np.arange(K, dtype=np.int32) | (c << _lib.MERGE_COMP_SHIFT) for c in range(3)])


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


nbytes = 48 * K * nvox
best, mean = timed(lambda: _lib.state_row_stats(ctx, src, K))
print(f"row_stats  nvox={nvox} K={K}: {best:.3f} ms best, {mean:.3f} ms mean per call; {nbytes / 1e6:.0f} MB read -> "
      f"{nbytes / best / 1e9 * 1e3:.0f} GB/s; at 6290 GB/s: {nbytes / 6.29e9:.3f} ms")
best, mean = timed(lambda: _lib.state_merge(ctx, dst, src, K, offsets, sources))
print(f"merge      nvox={nvox} K={K}: {best:.3f} ms best, {mean:.3f} ms mean per call; {2 * nbytes / 1e6:.0f} MB moved -> "
      f"{2 * nbytes / best / 1e9 * 1e3:.0f} GB/s")
grid = int(round(nvox ** 0.5))
sm = epg.StateMatrix(shape=(grid, grid), kgrid=1.0)
for op in [epg.T(90, 90)] + [epg.S(1.37), epg.T(np.linspace(100, 170, grid), 0)] * 10:
    sm = op(sm, inplace=True)
shift = epg.S(1.37)
t0 = time.perf_counter()
for _ in range(5):
    sm = shift(sm, inplace=True)
ctx.synchronize()
print(f"float shift nvox={grid * grid} nstate={sm.nstate}: {(time.perf_counter() - t0) / 5 * 1e3:.3f} ms per shift (op(sm), two downloads included)")

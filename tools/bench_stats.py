"""Cramer-Rao maps from a Jacobian left on the device (stats.crlb on a DeviceJacobian, crlb_kernel) against the route without
it: download the Jacobian, then the NumPy formula.

Workload: the 20-echo multi-spin-echo train over an n x n (T1, T2) grid (n = 1024: the grid of the headline benchmark) with
V = 1 (T2) and V = 3 (T2, T1, B1) derivative states, `Jacobian(["magnitude", ...])`, `out="device"`.

Per V, one JSON line:
  kernel_ms             device time of one epgx_signal_crlb launch (HIP events around `--steps` launches into one output buffer)
  bytes, bytes_per_s    nrec * P * 16 bytes read + 8 written per voxel (computed from the shapes), over kernel_ms
  share_of_copy_rate    bytes_per_s over 6.29e12 (the float4 copy rate of the part: the streaming ceiling)
  d2d_copy_bytes_per_s  a device-to-device copy of the Jacobian on this box (bytes read + written over its time), for the
                        same comparison on the same clocks
  device_ms             wall time of stats.crlb(jac_dev): allocation, launch, download of the map
  host_download_ms, host_numpy_ms   np.asarray(jac_dev), then stats.crlb on the array (one core of NumPy)
  max_rel_diff          device against host map (finite voxels)

    python tools/bench_stats.py [--n 1024] [--necho 20] [--steps 20] [--reps 5] [--skip-host] [--out profiles/stats_bench.jsonl]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from epgpy_amd import epg, stats, _lib  # noqa: E402

COPY_RATE = 6.29e12          # bytes/s, float4 copy on the MI355X (bytes read + written)


def jacobian_on_device(n, necho, variables):
    T1 = np.linspace(200, 3000, n)[:, None]
    T2 = np.linspace(20, 300, n)[None, :]
    exc = epg.T(90, 90, order1={"B1": {"alpha": 90}})
    rfc = epg.T(120, 0, order1={"B1": {"alpha": 120}})
    rlx = epg.E(5.0, T1, T2, order1=["T1", "T2"])
    seq = [exc] + [epg.S(1), rlx, rfc, epg.S(1), rlx, epg.ADC] * necho
    return epg.simulate(seq, probe=epg.Jacobian(["magnitude"] + variables), max_nstate=63, out="device")


def measure(args, variables):
    jac = jacobian_on_device(args.n, args.necho, variables)
    ctx = jac._buf.ctx
    P, nvox, nrec = len(jac.rows), jac.nvox, jac.nrec
    rows = np.ascontiguousarray(jac.rows, dtype=np.int32)
    out = _lib.DeviceBuffer(ctx, 8 * nvox, itemsize=8)

    def launch():
        _lib.check(ctx.lib.epgx_signal_crlb(ctx.handle, ctypes.c_void_p(jac.ptr), jac.record_stride, jac.row_stride, jac._nrow, nrec, P,
                                            rows.ctypes.data, 0, nvox, None, 1.0, 0, out.ptr), "epgx_signal_crlb")

    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.025:          # out of the idle clocks
        launch()
        ctx.synchronize()
    ctx.timer_start()
    for _ in range(args.steps):
        launch()
    kernel_ms = ctx.timer_stop() / args.steps
    nbytes = (16.0 * nrec * P + 8.0) * nvox

    jbytes = 16 * nrec * P * nvox
    scratch = _lib.DeviceBuffer(ctx, jbytes)
    copy = lambda: _lib.check(ctx.lib.epgx_memcpy_d2d(ctx.handle, scratch.ptr, ctypes.c_void_p(jac._buf.ptr.value), jbytes), "d2d")   # noqa: E731
    copy()
    ctx.synchronize()
    ctx.timer_start()
    for _ in range(args.steps):
        copy()
    copy_ms = ctx.timer_stop() / args.steps
    scratch.free()

    device = []
    for _ in range(args.reps):
        tic = time.perf_counter()
        got = stats.crlb(jac)
        device.append((time.perf_counter() - tic) * 1e3)
    res = dict(workload=f"mse {args.n}x{args.n}, {nrec} echoes", n_vars=len(variables), nparam=P, nvox=nvox, nrec=nrec,
               kernel_ms=kernel_ms, bytes=nbytes, bytes_per_s=nbytes / (kernel_ms * 1e-3),
               share_of_copy_rate=nbytes / (kernel_ms * 1e-3) / COPY_RATE,
               d2d_copy_ms=copy_ms, d2d_copy_bytes_per_s=2.0 * jbytes / (copy_ms * 1e-3),
               device_ms=float(np.median(device)), device_ms_all=[round(v, 3) for v in device], label=args.label)
    if not args.skip_host:
        tic = time.perf_counter()
        host = np.asarray(jac)
        res["host_download_ms"] = (time.perf_counter() - tic) * 1e3
        tic = time.perf_counter()
        with np.errstate(all="ignore"):
            want = stats.crlb(np.moveaxis(host, 0, -2))
        res["host_numpy_ms"] = (time.perf_counter() - tic) * 1e3
        ok = np.isfinite(want) & np.isfinite(got)
        res["finite_voxels"] = int(ok.sum())
        res["max_rel_diff"] = float(np.max(np.abs(got - want)[ok] / np.abs(want)[ok]))
    out.free()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--necho", type=int, default=20)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-host", action="store_true")
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    for variables in (["T2"], ["T2", "T1", "B1"]):
        line = json.dumps(measure(args, variables))
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as fh:
                fh.write(line + "\n")


if __name__ == "__main__":
    main()

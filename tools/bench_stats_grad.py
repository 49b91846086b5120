"""Cost and gradient of the Cramer-Rao bound from a Jacobian and second derivatives left on the device (stats.crlb_grad on a
DeviceJacobian and a DeviceHessian, crlb_grad_kernel) against the route without it: download both, then the NumPy formula.

Workload: synthetic device buffers in the layout a Jacobian probe and the passes of a Hessian call leave -- n x n voxels,
`nrec` records, P = 1 + V columns (magnitude first), nx design variables; the magnitude row of every pair is the first-order
row of its pass, the others the pass's last row (passes of 4 rows per record).  Seeded Gaussian records; nothing is simulated.

One JSON line:
  kernel_ms             device time of one epgx_signal_crlb_grad call (ceil(nx / 4) launches; HIP events around `--steps` calls)
  bytes, bytes_per_s    what the launches read and write, computed from the shapes: per voxel nrec * 16 bytes for every entry of
                        H that is present, nrec * P * 16 for J once per launch, 8 (1 + nx) written; over kernel_ms
  share_of_hbm_peak     bytes_per_s over 8e12 (the HBM peak of the part); share_of_copy_rate over 6.29e12 (float4 copy rate)
  device_ms             wall time of stats.crlb_grad(J_dev, H_dev): allocation, launches, download of the maps
  host_download_ms, host_numpy_ms   np.asarray of both handles, then stats.crlb(J, H=H) (one core of NumPy): the route of a
                        library without the device gradient
  max_err_over_scale    device against host gradient, largest |difference| over the largest |gradient| of the voxel

    python tools/bench_stats_grad.py [--n 256] [--nrec 20] [--nparam 2] [--nx 30] [--steps 20] [--reps 5] [--skip-host] [--out FILE]
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
from epgpy_amd import stats, functions, _lib  # noqa: E402

HBM_PEAK = 8.0e12            # bytes/s
COPY_RATE = 6.29e12          # bytes/s, float4 copy on the MI355X (bytes read + written)


def fill(ctx, nelem, seed):
    """a device buffer of nelem complex128 standard-normal values (uploaded in blocks)"""
    buf = _lib.DeviceBuffer(ctx, 16 * nelem)
    rng = np.random.default_rng(seed)
    block = 1 << 24
    for start in range(0, nelem, block):
        n = min(block, nelem - start)
        part = (rng.standard_normal(2 * n)).view(np.complex128)
        _lib.check(ctx.lib.epgx_memcpy_h2d(ctx.handle, ctypes.c_void_p(buf.ptr.value + 16 * start), part.ctypes.data, part.nbytes), "h2d")
    return buf


def handles(ctx, n, nrec, nparam, nx):
    grid = (n, n)
    nvox = n * n
    params = ["magnitude"] + [f"p{c}" for c in range(1, nparam)]
    design = [f"x{x}" for x in range(nx)]
    jac = functions.DeviceJacobian(fill(ctx, nrec * nparam * nvox, 1), nrec, grid, 1, nparam, 0, list(range(nparam)), params)
    # one pass per (parameter, design variable) pair, 4 rows per record; with one parameter the magnitude reads row 2 of pass x
    pairs = [(p, x) for p in params[1:] for x in design] or [("none", x) for x in design]
    layout = functions._HessianLayout(pairs, nrec * 4, 1, grid, nrec)
    where = np.zeros((nparam, nx, 2), dtype=np.int64)
    for x in range(nx):
        where[0, x] = (x, 2)
        for c in range(1, nparam):
            where[c, x] = ((c - 1) * nx + x, 3)
    hes = functions.DeviceHessian(fill(ctx, len(pairs) * nrec * 4 * nvox, 2), layout, where, params, design)
    return jac, hes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--nrec", type=int, default=20)
    ap.add_argument("--nparam", type=int, default=2)
    ap.add_argument("--nx", type=int, default=30)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-host", action="store_true")
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    ctx = _lib.get_context(0)
    jac, hes = handles(ctx, args.n, args.nrec, args.nparam, args.nx)
    P, nx, nvox, nrec = args.nparam, args.nx, jac.nvox, args.nrec
    rows = np.ascontiguousarray(jac.rows, dtype=np.int32)
    off = np.ascontiguousarray(hes.offsets, dtype=np.int64)
    step = np.ascontiguousarray(hes.record_strides, dtype=np.int64)
    out = _lib.DeviceBuffer(ctx, 8 * (1 + nx) * nvox, itemsize=8)

    def launch():
        _lib.check(ctx.lib.epgx_signal_crlb_grad(ctx.handle, ctypes.c_void_p(jac.ptr), jac.record_stride, jac.row_stride, jac._nrow, nrec, P,
                                                 rows.ctypes.data, 0, nvox, ctypes.c_void_p(hes.ptr), hes._buf.nbytes // 16, nx,
                                                 off.ctypes.data, step.ctypes.data, None, 1.0, 0, out.ptr,
                                                 ctypes.c_void_p(out.ptr.value + 8 * nvox)), "epgx_signal_crlb_grad")

    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.05:           # out of the idle clocks
        launch()
        ctx.synchronize()
    ctx.timer_start()
    for _ in range(args.steps):
        launch()
    kernel_ms = ctx.timer_stop() / args.steps
    with open(os.path.join(ROOT, "epgpy_amd", "csrc", "epgx_stats.h")) as fh:
        xb = int(fh.read().split("constexpr int CRLB_GRAD_XB = ")[1].split(";")[0])
    launches = -(-nx // xb)
    nbytes = (16.0 * nrec * int((off >= 0).sum()) + 16.0 * nrec * P * launches + 8.0 * (1 + nx)) * nvox
    rate = nbytes / (kernel_ms * 1e-3)

    device = []
    for _ in range(args.reps):
        tic = time.perf_counter()
        cost, grad = stats.crlb_grad(jac, hes)
        device.append((time.perf_counter() - tic) * 1e3)
    res = dict(workload=f"{args.n}x{args.n} voxels, {nrec} records, P = {P}, nx = {nx}", nvox=nvox, nrec=nrec, nparam=P, nx=nx,
               hessian_bytes=hes._buf.nbytes, launches=launches, kernel_ms=kernel_ms, bytes=nbytes, bytes_per_s=rate,
               share_of_hbm_peak=rate / HBM_PEAK, share_of_copy_rate=rate / COPY_RATE,
               device_ms=float(np.median(device)), device_ms_all=[round(v, 3) for v in device], label=args.label)
    if not args.skip_host:
        tic = time.perf_counter()
        J, H = np.asarray(jac), np.asarray(hes)
        res["host_download_ms"] = (time.perf_counter() - tic) * 1e3
        tic = time.perf_counter()
        with np.errstate(all="ignore"):
            _, want = stats.crlb(np.moveaxis(J, 0, -2), H=np.moveaxis(H, 0, -3))
        res["host_numpy_ms"] = (time.perf_counter() - tic) * 1e3
        ok = np.isfinite(want).all(-1) & np.isfinite(grad).all(-1)
        scale = np.abs(want[ok]).max(-1, keepdims=True)
        res["finite_voxels"] = int(ok.sum())
        res["max_err_over_scale"] = float(np.max(np.abs(grad[ok] - want[ok]) / scale))
    out.free()
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()

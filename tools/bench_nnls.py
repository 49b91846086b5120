"""Non-negative mixtures on the device (epgx_signal_nnls: nnls_kernel, csrc/epgx_nnls.hip) and, for scale, the same problem through
`scipy.optimize.nnls` on the host cores.

Workload: an analytic multi-echo dictionary, D[t, a, g] = exp(-(t + 1) ESP / T2_a) times an alternating, decaying modulation per
group g (what a B1 error does to the odd and even echoes), `--nt2` T2 values from 10 to 2000 ms x `--nb1` groups x `--nrec`
echoes; signals: two-pool voxels (20 and 80 ms, a random share and group) with complex noise.  Nothing is simulated.
The kernel is timed by device events around the raw entry after one warm-up call, `--reps` calls; median, min and max.  A task is
one (voxel, group) pair: nmeas x nb1 of them per call.  The host route solves `--host-voxels` voxels in every group on the stacked
real system with a pool of `--procs` processes, wall clock, and is scaled to tasks per second.

One JSON line:
  kernel_ms (median), tasks, tasks_per_s, gram_ms (upload of the dictionary and its Gram matrices, once per dictionary), status (voxels at 0 / 1 / 2),
  scipy_tasks_per_s, procs, ratio = tasks_per_s / scipy_tasks_per_s, agree = max |w_device - w_scipy| / max |w_scipy| in the chosen group

    python tools/bench_nnls.py [--nt2 40] [--nb1 16] [--nrec 32] [--nmeas 65536] [--reps 5] [--host-voxels 64] [--procs 16] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def dictionary(nt2, nb1, nrec, esp=10.0):
    t2 = np.geomspace(10.0, 2000.0, nt2)
    t = np.arange(1, nrec + 1, dtype=np.float64)
    atoms = np.exp(-t[:, None] * esp / t2[None, :])
    mod = 1.0 + 0.35 * ((np.arange(nb1) + 1.0) / nb1)[None, :] * ((-1.0) ** t * np.exp(-0.15 * t))[:, None]
    return t2, (atoms[:, :, None] * mod[:, None, :]).astype(np.complex128)      # [nrec, nt2, nb1]


def two_pools(D, t2, nmeas, seed=0, esp=10.0):
    rng = np.random.default_rng(seed)
    nrec, _, nb1 = D.shape
    t = np.arange(1, nrec + 1, dtype=np.float64)
    mod = D[:, 0, :].real / np.exp(-t * esp / t2[0])[:, None]
    grp = rng.integers(0, nb1, nmeas)
    share = rng.uniform(0.05, 0.25, nmeas)
    S = (share[None, :] * np.exp(-t * esp / 20.0)[:, None] + (1 - share)[None, :] * np.exp(-t * esp / 80.0)[:, None]) * mod[:, grp]
    return S + 1e-3 * (rng.standard_normal(S.shape) + 1j * rng.standard_normal(S.shape))


def _scipy_voxel(args):
    from scipy.optimize import nnls
    stacked, rhs = args
    return [nnls(M, rhs, maxiter=30 * M.shape[1])[0] for M in stacked]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nt2", type=int, default=40)
    ap.add_argument("--nb1", type=int, default=16)
    ap.add_argument("--nrec", type=int, default=32)
    ap.add_argument("--nmeas", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-voxels", type=int, default=64)
    ap.add_argument("--procs", type=int, default=16)
    ap.add_argument("--reg", type=float, default=1e-8)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    t2, D = dictionary(args.nt2, args.nb1, args.nrec)
    S = two_pools(D, t2, args.nmeas)

    # the host route first, in processes that never open the GPU
    nhost = min(args.host_voxels, args.nmeas)
    n = (np.abs(D) ** 2).sum(axis=0)                                            # [nt2, nb1]
    mu = args.reg * n.mean(axis=0)
    stacked = [np.concatenate([D[:, :, g].real, D[:, :, g].imag, np.sqrt(mu[g]) * np.eye(args.nt2)], axis=0) for g in range(args.nb1)]
    jobs = [(stacked, np.concatenate([S[:, m].real, S[:, m].imag, np.zeros(args.nt2)])) for m in range(nhost)]
    import multiprocessing
    with multiprocessing.get_context("spawn").Pool(args.procs) as pool:
        pool.map(_scipy_voxel, jobs[:args.procs])                                # (start-up and imports out of the clock)
        t0 = time.perf_counter()
        ref = pool.map(_scipy_voxel, jobs)
        host_s = time.perf_counter() - t0
    scipy_rate = nhost * args.nb1 / host_s

    from epgpy_amd import _lib, match
    ctx = _lib.get_context(0)
    ctx.timer_start()
    comp = match.Components(D, 0)
    gram_ms = ctx.timer_stop()
    sig = _lib.DeviceBuffer(ctx, S.nbytes)
    sig.upload(S)
    rec = comp._rec

    import ctypes
    out = _lib.DeviceBuffer(ctx, 8 * (args.nt2 + 3) * args.nmeas, itemsize=8)
    base, V, A, N = out.ptr.value, ctypes.c_void_p, args.nt2, args.nmeas

    def kernel():
        _lib.check(ctx.lib.epgx_signal_nnls(ctx.handle, V(rec.ptr), rec.row_stride, comp.nrec, A, comp._ninner, comp._nouter, comp._ninner,
                                            comp._gram.ptr, comp._mask.ptr, sig.ptr, N, N, args.reg, match.NNLS_TOL, None, V(base),
                                            V(base + 8 * A * N), V(base + 8 * (A + 1) * N), V(base + 8 * (A + 2) * N)), "epgx_signal_nnls")

    kernel()
    ctx.synchronize()
    ms = []
    for _ in range(args.reps):
        ctx.timer_start()
        kernel()
        ms.append(ctx.timer_stop())
    raw = out.download(np.float64, ((A + 3) * N,))          # what the last timed call wrote
    weights, group, status = raw[:A * N].reshape(A, N), raw[A * N:(A + 1) * N].view(np.int64), raw[(A + 2) * N:].view(np.int32)[:N]
    tasks = args.nmeas * args.nb1
    agree = max(float(np.max(np.abs(weights[:, m] - ref[m][int(group[m])]))) for m in range(nhost)) / \
        max(float(np.max(np.abs(ref[m][int(group[m])]))) for m in range(nhost))
    res = dict(nt2=args.nt2, nb1=args.nb1, nrec=args.nrec, nmeas=args.nmeas, reg=args.reg, reps=args.reps, kernel_ms=float(np.median(ms)),
               kernel_ms_min=float(np.min(ms)), kernel_ms_max=float(np.max(ms)), tasks=tasks, tasks_per_s=tasks / (np.median(ms) * 1e-3),
               gram_ms=gram_ms, status=np.bincount(status, minlength=3).tolist(), scipy_tasks_per_s=scipy_rate, procs=args.procs,
               host_voxels=nhost, ratio=tasks / (np.median(ms) * 1e-3) / scipy_rate, agree=agree)
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()

"""The chi^2-driven ridge on the device (epgx_signal_nnls_chi2: nnls_kernel, then nnls_chi2_kernel of csrc/epgx_nnls_chi2.hip) against
the plain fit (epgx_signal_nnls) on the same inputs in the same process and, for scale, the same fits through
`scipy.optimize.nnls` inside `scipy.optimize.brentq` on the host cores.

Workload: the dictionary and the two-pool voxels of tools/bench_nnls.py.  Every call is timed by device events around the raw
entry after one warm-up call, `--reps` calls; median, min and max.  Four calls: the plain fit with the group search, the chi2
call with the group search, and both with the groups fixed to the ones found (the chi2 kernel's own share: one fit per
evaluation in ONE group).  The host route solves `--host-voxels` voxels: the unregularised fit in every group, then brentq on
log mu in the best group, in a pool of `--procs` processes, wall clock.

The model to test: chi2 call (fixed groups) ~ (1 + mean evals x growth of a solve with the larger passive set) x the plain call
with fixed groups.  `model_solve_growth` is the growth that would make the model exact; the passive-set sizes are printed next
to it.

One JSON line:
  plain_ms, chi2_ms, plain_fixed_ms, chi2_fixed_ms (medians, with _min and _max), ratio = chi2_ms / plain_ms, ratio_fixed,
  evals_hist, evals_mean, passive_hist (final, regularised), passive_plain_hist, status (voxels at 0 .. 4),
  model_solve_growth = (ratio_fixed - 1) / evals_mean, host_fits_per_s, fits_per_s (voxels per second of the chi2 call)

    python tools/bench_nnls_chi2.py [--nt2 40] [--nb1 16] [--nrec 32] [--nmeas 65536] [--chi2 1.02] [--reps 5] [--host-voxels 64]
                                    [--procs 16] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_nnls import dictionary, two_pools      # noqa: E402


def _host_voxel(args):
    """the unregularised fit in every group, then brentq on log mu in the best one: (group, mu, weights)"""
    from scipy.optimize import brentq, nnls
    D, mu0, s, chi2 = args
    nrec, A, G = D.shape
    rhs = np.concatenate([s.real, s.imag, np.zeros(A)])

    def fit(g, mu):
        M = np.concatenate([D[:, :, g].real, D[:, :, g].imag, np.sqrt(mu) * np.eye(A)], axis=0)
        x = nnls(M, rhs, maxiter=30 * A)[0]
        return x, float(np.sum(np.abs(s - D[:, :, g] @ x) ** 2))

    best = min(range(G), key=lambda g: fit(g, mu0[g])[1] + mu0[g] * float(np.sum(fit(g, mu0[g])[0] ** 2)))
    T = chi2 * fit(best, mu0[best])[1]
    r = lambda t: fit(best, np.exp(t))[1] / T - 1      # noqa: E731
    lo = np.log(mu0[best])
    hi = lo + np.log(16.0)
    while r(hi) < 0:
        lo, hi = hi, hi + np.log(16.0)
    t = brentq(r, lo, hi, xtol=1e-6, rtol=1e-8)
    return best, float(np.exp(t)), fit(best, np.exp(t))[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nt2", type=int, default=40)
    ap.add_argument("--nb1", type=int, default=16)
    ap.add_argument("--nrec", type=int, default=32)
    ap.add_argument("--nmeas", type=int, default=65536)
    ap.add_argument("--chi2", type=float, default=1.02)
    ap.add_argument("--rtol", type=float, default=1e-3)
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
    mu0 = args.reg * (np.abs(D) ** 2).sum(axis=0).mean(axis=0)
    jobs = [(D, mu0, S[:, m], args.chi2) for m in range(nhost)]
    import multiprocessing
    with multiprocessing.get_context("spawn").Pool(args.procs) as pool:
        pool.map(_host_voxel, jobs[:args.procs])                                 # (start-up and imports out of the clock)
        t0 = time.perf_counter()
        ref = pool.map(_host_voxel, jobs)
        host_s = time.perf_counter() - t0

    import ctypes
    from epgpy_amd import _lib, match
    ctx = _lib.get_context(0)
    comp = match.Components(D, 0)
    sig = _lib.DeviceBuffer(ctx, S.nbytes)
    sig.upload(S)
    rec = comp._rec
    V, A, N = ctypes.c_void_p, args.nt2, args.nmeas
    out = _lib.DeviceBuffer(ctx, 8 * (A + 5) * N, itemsize=8)
    grp = _lib.DeviceBuffer(ctx, 8 * N, itemsize=8)
    base = out.ptr.value
    row = lambda i: V(base + 8 * (A + i) * N)      # noqa: E731
    common = (ctx.handle, V(rec.ptr), rec.row_stride, comp.nrec, A, comp._ninner, comp._nouter, comp._ninner, comp._gram.ptr, comp._mask.ptr,
              sig.ptr, N, N, args.reg, match.NNLS_TOL)

    def plain(group=None):
        _lib.check(ctx.lib.epgx_signal_nnls(*common, group, V(base), row(0), row(1), row(4)), "epgx_signal_nnls")

    def chi2(group=None):
        _lib.check(ctx.lib.epgx_signal_nnls_chi2(*common, group, args.chi2, args.rtol, _lib.NNLS_CHI2_EVALS, V(base), row(0), row(1), row(4),
                                                 row(2), row(3), V(base + 8 * (A + 4) * N + 4 * N)), "epgx_signal_nnls_chi2")

    def timed(call, *a):
        call(*a)
        ctx.synchronize()
        ms = []
        for _ in range(args.reps):
            ctx.timer_start()
            call(*a)
            ms.append(ctx.timer_stop())
        return dict(median=float(np.median(ms)), min=float(np.min(ms)), max=float(np.max(ms)))

    t_plain = timed(plain)
    raw = out.download(np.float64, ((A + 5) * N,))
    w_plain, found = raw[:A * N].reshape(A, N).copy(), raw[A * N:(A + 1) * N].view(np.int64).copy()
    grp.upload(found)
    t_plain_fixed = timed(plain, grp.ptr)
    t_chi2_fixed = timed(chi2, grp.ptr)
    t_chi2 = timed(chi2)
    raw = out.download(np.float64, ((A + 5) * N,))          # what the last timed call wrote
    weights, group = raw[:A * N].reshape(A, N), raw[A * N:(A + 1) * N].view(np.int64)
    mu = raw[(A + 2) * N:(A + 3) * N]
    ints = raw[(A + 4) * N:].view(np.int32)
    status, evals = ints[:N], ints[N:2 * N]
    agree_group = float(np.mean([int(group[m]) == ref[m][0] for m in range(nhost)]))
    agree_mu = float(np.max([abs(np.log(mu[m] / ref[m][1])) for m in range(nhost) if int(group[m]) == ref[m][0] and status[m] == 0] or [np.nan]))
    ratio_fixed = t_chi2_fixed["median"] / t_plain_fixed["median"]
    res = dict(nt2=args.nt2, nb1=args.nb1, nrec=args.nrec, nmeas=N, reg=args.reg, chi2=args.chi2, chi2_rtol=args.rtol, reps=args.reps,
               plain_ms=t_plain["median"], plain_ms_min=t_plain["min"], plain_ms_max=t_plain["max"],
               chi2_ms=t_chi2["median"], chi2_ms_min=t_chi2["min"], chi2_ms_max=t_chi2["max"],
               plain_fixed_ms=t_plain_fixed["median"], plain_fixed_ms_min=t_plain_fixed["min"], plain_fixed_ms_max=t_plain_fixed["max"],
               chi2_fixed_ms=t_chi2_fixed["median"], chi2_fixed_ms_min=t_chi2_fixed["min"], chi2_fixed_ms_max=t_chi2_fixed["max"],
               ratio=t_chi2["median"] / t_plain["median"], ratio_fixed=ratio_fixed,
               evals_hist=np.bincount(evals).tolist(), evals_mean=float(evals.mean()),
               passive_hist=np.bincount((weights > 0).sum(axis=0)).tolist(), passive_plain_hist=np.bincount((w_plain > 0).sum(axis=0)).tolist(),
               status=np.bincount(status, minlength=5).tolist(), model_solve_growth=(ratio_fixed - 1) / max(float(evals.mean()), 1e-30),
               fits_per_s=N / (t_chi2["median"] * 1e-3), host_fits_per_s=nhost / host_s, procs=args.procs, host_voxels=nhost,
               host_group_agree=agree_group, host_log_mu_diff=agree_mu)
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()

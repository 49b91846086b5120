"""SVD compression of a device dictionary (epgx_signal_gram: gram_kernel + gram_reduce_kernel, epgx_signal_project:
project_kernel, csrc/epgx_compress.hip) against torch on the same GPU.

    python tools/bench_compress.py [--natoms A] [--reps R] [--nmeas M] [--skip-pipeline] [--out FILE]

Seeded Gaussian dictionaries generated on the device; device events around whole entry-point calls, one warm-up, median of
`reps` (default 3), alternating with the baseline.  One JSON line per point:
  what="gram"      nrec 64 and 1000: gram_ms against torch complex128 `D @ D.conj().T`, flop/s at 4 nrec^2 natoms flop (the
                   Hermitian half) and the share of the 78.6 TFLOP/s fp64 peak, the largest difference of the two results
  what="project"   ranks 8, 16, 64 at 1000 records: project_ms against torch `U^H @ D` and against norms_ms, the time
                   norms_kernel takes to read the same dictionary (the HBM yardstick), bytes/s at 16 nrec natoms bytes
  what="pipeline"  1000 records: compress once (Gram, eigh on the host, projection at rank 16) plus epgx_signal_match at rank 16
                   over nmeas voxels, against the uncompressed epgx_signal_match at the same shapes
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
from epgpy_amd import _lib, match  # noqa: E402

FP64_PEAK = 78.6e12          # flop/s, vector = matrix on the MI355X
P = ctypes.c_void_p


def stats(values):
    return dict(median=float(np.median(values)), min=float(np.min(values)), max=float(np.max(values)))


def alternate(torch, ctx, dev, ours, theirs, reps):
    """one warm-up each, then `reps` alternating timings: (ours_ms, theirs_ms)"""
    def timed(fn):
        ctx.timer_start()
        fn()
        return ctx.timer_stop()

    def timed_torch(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        torch.cuda.synchronize(dev)
        return t0.elapsed_time(t1)

    ours()
    ctx.synchronize()
    if theirs is not None:
        theirs()
        torch.cuda.synchronize(dev)
    a, b = [], []
    for _ in range(reps):
        a.append(timed(ours))
        if theirs is not None:
            b.append(timed_torch(theirs))
    return a, b


def emit(res, out):
    line = json.dumps(res)
    print(line, flush=True)
    if out:
        with open(out, "a") as fh:
            fh.write(line + "\n")


def dictionary(torch, dev, nrec, natoms, seed=0):
    gen = torch.Generator(device=dev)
    gen.manual_seed(seed)
    D = torch.view_as_complex(torch.randn((nrec, natoms, 2), dtype=torch.float64, device=dev, generator=gen))
    torch.cuda.synchronize(dev)
    return D


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--natoms", type=int, default=1000000)
    ap.add_argument("--nmeas", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--skip-pipeline", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_compress: no GPU visible; this tool measures on the device only")
    ctx = _lib.get_context(0)
    dev = torch.device("cuda", ctx.device)
    natoms, reps = args.natoms, args.reps

    for nrec in (64, 1000):
        D = dictionary(torch, dev, nrec, natoms)
        norms = _lib.signal_norms(ctx, D.data_ptr(), natoms, nrec, natoms)
        G = _lib.DeviceBuffer(ctx, 16 * nrec * nrec)
        keep = {}

        def run_gram():
            _lib.check(ctx.lib.epgx_signal_gram(ctx.handle, P(D.data_ptr()), natoms, norms.ptr, nrec, natoms, 0, G.ptr), "epgx_signal_gram")

        def run_torch():
            keep["G"] = torch.matmul(D, D.conj().T)

        ours, theirs = alternate(torch, ctx, dev, run_gram, run_torch, reps)
        flop = 4.0 * nrec * nrec * natoms
        o, t = stats(ours), stats(theirs)
        got = G.download(np.complex128, (nrec, nrec))
        ref = keep["G"].cpu().numpy()
        emit(dict(what="gram", natoms=natoms, nrec=nrec, nsplit=_lib.gram_nsplit(nrec, natoms), reps=reps, gram_ms=o["median"],
                  gram_ms_min=o["min"], gram_ms_max=o["max"], gram_flops=flop / (o["median"] * 1e-3),
                  gram_share_of_fp64_peak=flop / (o["median"] * 1e-3) / FP64_PEAK, torch_ms=t["median"], torch_ms_min=t["min"],
                  torch_ms_max=t["max"], torch_flops_hermitian_half=flop / (t["median"] * 1e-3), speedup=t["median"] / o["median"],
                  max_rel_diff=float(np.abs(got - ref).max() / np.abs(ref).max())), args.out)
        G.free()
        if nrec != 1000:
            norms.free()
            del D, keep
            torch.cuda.empty_cache()

    # D: 1000 records; the basis from its own Gram matrix
    nrec = 1000
    t0 = time.perf_counter()
    U, lam = match.gram_basis(got)
    eigh_s = time.perf_counter() - t0

    def run_norms():
        _lib.check(ctx.lib.epgx_signal_norms(ctx.handle, P(D.data_ptr()), natoms, nrec, natoms, norms.ptr), "epgx_signal_norms")

    norms_ms = stats(alternate(torch, ctx, dev, run_norms, None, reps)[0])["median"]
    project_ms = {}
    for rank in (8, 16, 64):
        B = np.ascontiguousarray(U[:, :rank])
        bbuf = _lib.DeviceBuffer(ctx, B.nbytes)
        bbuf.upload(B)
        out = _lib.DeviceBuffer(ctx, 16 * rank * natoms)
        tB = torch.from_numpy(B).to(dev)

        def run_project():
            _lib.check(ctx.lib.epgx_signal_project(ctx.handle, bbuf.ptr, rank, P(D.data_ptr()), natoms, nrec, natoms, out.ptr, natoms),
                       "epgx_signal_project")

        def run_torch():
            keep["Dc"] = torch.matmul(tB.conj().T, D)

        ours, theirs = alternate(torch, ctx, dev, run_project, run_torch, reps)
        o, t = stats(ours), stats(theirs)
        project_ms[rank] = o["median"]
        nbytes, flop = 16.0 * nrec * natoms, 8.0 * rank * nrec * natoms
        emit(dict(what="project", natoms=natoms, nrec=nrec, rank=rank, reps=reps, project_ms=o["median"], project_ms_min=o["min"],
                  project_ms_max=o["max"], project_bytes_per_s=nbytes / (o["median"] * 1e-3), project_flops=flop / (o["median"] * 1e-3),
                  project_share_of_fp64_peak=flop / (o["median"] * 1e-3) / FP64_PEAK, norms_ms=norms_ms,
                  norms_bytes_per_s=nbytes / (norms_ms * 1e-3), against_norms=norms_ms / o["median"], torch_ms=t["median"],
                  torch_ms_min=t["min"], torch_ms_max=t["max"], speedup=t["median"] / o["median"]), args.out)
        if rank != 16 or args.skip_pipeline:
            out.free()
        else:
            Dc = out
        bbuf.free()
        del tB
        keep.clear()
        torch.cuda.empty_cache()

    if args.skip_pipeline:
        return
    # compress once + match at rank 16, against the uncompressed match
    rank, nmeas = 16, args.nmeas
    gram_ms = None
    S = dictionary(torch, dev, nrec, nmeas, seed=1)
    B = np.ascontiguousarray(U[:, :rank])
    bbuf = _lib.DeviceBuffer(ctx, B.nbytes)
    bbuf.upload(B)
    Sc = _lib.DeviceBuffer(ctx, 16 * rank * nmeas)
    cnorms = _lib.signal_norms(ctx, Dc.ptr.value, natoms, rank, natoms)
    res = _lib.DeviceBuffer(ctx, 32 * nmeas, itemsize=8)

    def run_gram():
        g = _lib.signal_gram(ctx, D.data_ptr(), natoms, norms.ptr.value, nrec, natoms)
        g.free()

    def run_signals():
        _lib.check(ctx.lib.epgx_signal_project(ctx.handle, bbuf.ptr, rank, P(S.data_ptr()), nmeas, nrec, nmeas, Sc.ptr, nmeas), "epgx_signal_project")

    def run_cnorms():
        _lib.check(ctx.lib.epgx_signal_norms(ctx.handle, Dc.ptr, natoms, rank, natoms, cnorms.ptr), "epgx_signal_norms")

    def run_cmatch():
        _lib.check(ctx.lib.epgx_signal_match(ctx.handle, Dc.ptr, natoms, cnorms.ptr, natoms, Sc.ptr, nmeas, rank, nmeas, 0,
                                             P(res.ptr.value + 16 * nmeas), res.ptr, P(res.ptr.value + 24 * nmeas)), "epgx_signal_match")

    def run_match():
        _lib.check(ctx.lib.epgx_signal_match(ctx.handle, P(D.data_ptr()), natoms, norms.ptr, natoms, P(S.data_ptr()), nmeas, nrec, nmeas, 0,
                                             P(res.ptr.value + 16 * nmeas), res.ptr, P(res.ptr.value + 24 * nmeas)), "epgx_signal_match")

    med = lambda fn: stats(alternate(torch, ctx, dev, fn, None, reps)[0])["median"]      # noqa: E731
    gram_ms, signals_ms, cnorms_ms, cmatch_ms = med(run_gram), med(run_signals), med(run_cnorms), med(run_cmatch)
    cindex = res.download(np.float64, (4 * nmeas,))[2 * nmeas:3 * nmeas].view(np.int64).copy()
    match_ms = med(run_match)
    index = res.download(np.float64, (4 * nmeas,))[2 * nmeas:3 * nmeas].view(np.int64)
    once = gram_ms + 1e3 * eigh_s + project_ms[rank] + cnorms_ms
    emit(dict(what="pipeline", natoms=natoms, nmeas=nmeas, nrec=nrec, rank=rank, reps=reps, gram_ms=gram_ms, eigh_host_ms=1e3 * eigh_s,
              project_dictionary_ms=project_ms[rank], compressed_norms_ms=cnorms_ms, compress_once_ms=once,
              project_signals_ms=signals_ms, compressed_match_ms=cmatch_ms, per_call_ms=signals_ms + cmatch_ms,
              first_call_ms=once + signals_ms + cmatch_ms, uncompressed_match_ms=match_ms,
              speedup_first_call=match_ms / (once + signals_ms + cmatch_ms), speedup_per_call=match_ms / (signals_ms + cmatch_ms),
              same_atom=float(np.mean(index == cindex)),
              note="Gaussian data has no low-rank structure: same_atom says nothing about accuracy, the times do not depend on the data"),
         args.out)


if __name__ == "__main__":
    main()

"""Dictionary matching on the device (epgx_signal_match: match_kernel + match_merge_kernel, csrc/epgx_match.hip) against the
route without it on the same GPU: a chunked torch complex128 matmul + abs^2 + argmax that writes every chunk of the correlation
matrix to HBM and reads it back.

Workload: seeded complex Gaussian dictionary [nrec][natoms] and signals [nrec][nmeas], generated on the device (torch); nothing
is simulated.  The library reads torch's buffers through their addresses; both sides are timed with device events around whole
calls, after one warm-up call each, `--reps` calls each, alternating; median, min and max are reported.

One JSON line per point:
  pairs                 natoms * nmeas
  fused_ms              epgx_signal_match (norms excluded: once per dictionary; norms_ms next to it)
  fused_pairs_per_s, fused_flops, fused_share_of_fp64_peak     8 * nrec flop per pair over fused_ms, over 78.6e12
  torch_ms              the chunked baseline (chunks of --chunk-gb of correlation matrix), torch_pairs_per_s, torch_flops
  speedup               torch_ms / fused_ms
  agree                 share of voxels where both return the same atom (Gaussian data: no ties)

    python tools/bench_match.py                          # the suite of DESIGN 4.11
    python tools/bench_match.py --natoms 65536 --nmeas 65536 --nrec 16 [--reps 5] [--chunk-gb 2] [--skip-torch] [--out FILE]

The suite: natoms = 65 536 and 10^6, nmeas = 65 536, nrec = 16, 64, 1000 -- the 10^6 x 1000 point at nmeas = 8192 (8.2e9 pairs of
8000 flop: seconds per call at any rate either side reaches; the full 65 536 voxels are eight such calls).
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from epgpy_amd import _lib  # noqa: E402

FP64_PEAK = 78.6e12          # flop/s, vector = matrix on the MI355X

SUITE = [(65536, 65536, 16), (65536, 65536, 64), (65536, 65536, 1000), (1000000, 65536, 16), (1000000, 65536, 64), (1000000, 8192, 1000)]


def torch_match(torch, D, S, norms, chunk_atoms):
    """running argmax over chunks of atoms: C = D_chunk^H S, q = |C|^2 / n"""
    nmeas = S.shape[1]
    best = torch.full((nmeas,), -1.0, dtype=torch.float64, device=S.device)
    index = torch.full((nmeas,), -1, dtype=torch.int64, device=S.device)
    for a0 in range(0, D.shape[1], chunk_atoms):
        a1 = min(a0 + chunk_atoms, D.shape[1])
        C = torch.matmul(D[:, a0:a1].conj().T, S)                     # [chunk, nmeas] complex128 through HBM
        q = (C.real ** 2 + C.imag ** 2) / norms[a0:a1, None]
        val, arg = torch.max(q, dim=0)
        take = val > best
        best = torch.where(take, val, best)
        index = torch.where(take, arg + a0, index)
    return index


def stats(values):
    return dict(median=float(np.median(values)), min=float(np.min(values)), max=float(np.max(values)))


def point(torch, ctx, natoms, nmeas, nrec, reps, chunk_gb, skip_torch, seed=0):
    dev = torch.device("cuda", ctx.device)
    gen = torch.Generator(device=dev)
    gen.manual_seed(seed)
    D = torch.view_as_complex(torch.randn((nrec, natoms, 2), dtype=torch.float64, device=dev, generator=gen))
    S = torch.view_as_complex(torch.randn((nrec, nmeas, 2), dtype=torch.float64, device=dev, generator=gen))
    torch.cuda.synchronize(dev)
    norms = _lib.DeviceBuffer(ctx, 8 * natoms, itemsize=8)
    out = _lib.DeviceBuffer(ctx, 32 * nmeas, itemsize=8)
    P = ctypes.c_void_p

    def run_norms():
        _lib.check(ctx.lib.epgx_signal_norms(ctx.handle, P(D.data_ptr()), natoms, nrec, natoms, norms.ptr), "epgx_signal_norms")

    def run_fused():
        _lib.check(ctx.lib.epgx_signal_match(ctx.handle, P(D.data_ptr()), natoms, norms.ptr, natoms, P(S.data_ptr()), nmeas, nrec, nmeas, 0,
                                             P(out.ptr.value + 16 * nmeas), out.ptr, P(out.ptr.value + 24 * nmeas)), "epgx_signal_match")

    def timed(fn):
        ctx.timer_start()
        fn()
        return ctx.timer_stop()

    run_norms()
    run_fused()
    ctx.synchronize()
    norms_ms = [timed(run_norms) for _ in range(reps)]
    tnorms = torch.from_numpy(norms.download(np.float64, (natoms,))).to(dev)
    chunk_atoms = max(int(chunk_gb * 2 ** 30 // (16 * nmeas)), 16)
    fused_ms, torch_ms, tindex = [], [], None
    if not skip_torch:
        tindex = torch_match(torch, D, S, tnorms, chunk_atoms)       # warm-up: rocBLAS picks its kernels
        torch.cuda.synchronize(dev)
    for _ in range(reps):                                             # alternating
        fused_ms.append(timed(run_fused))
        if not skip_torch:
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            tindex = torch_match(torch, D, S, tnorms, chunk_atoms)
            t1.record()
            torch.cuda.synchronize(dev)
            torch_ms.append(t0.elapsed_time(t1))
    pairs = natoms * nmeas
    flop = 8.0 * nrec * pairs
    f = stats(fused_ms)
    res = dict(natoms=natoms, nmeas=nmeas, nrec=nrec, pairs=pairs, reps=reps, norms_ms=stats(norms_ms)["median"],
               fused_ms=f["median"], fused_ms_min=f["min"], fused_ms_max=f["max"],
               fused_pairs_per_s=pairs / (f["median"] * 1e-3), fused_flops=flop / (f["median"] * 1e-3),
               fused_share_of_fp64_peak=flop / (f["median"] * 1e-3) / FP64_PEAK)
    if not skip_torch:
        t = stats(torch_ms)
        index = out.download(np.float64, (4 * nmeas,))[2 * nmeas:3 * nmeas].view(np.int64)
        res.update(torch_chunk_atoms=chunk_atoms, torch_ms=t["median"], torch_ms_min=t["min"], torch_ms_max=t["max"],
                   torch_pairs_per_s=pairs / (t["median"] * 1e-3), torch_flops=flop / (t["median"] * 1e-3),
                   speedup=t["median"] / f["median"], agree=float(np.mean(index == tindex.cpu().numpy())))
    norms.free()
    out.free()
    del D, S
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--natoms", type=int, default=0)
    ap.add_argument("--nmeas", type=int, default=65536)
    ap.add_argument("--nrec", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--chunk-gb", type=float, default=2.0)
    ap.add_argument("--skip-torch", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_match: no GPU visible; this tool measures on the device only")
    ctx = _lib.get_context(0)
    points = [(args.natoms, args.nmeas, args.nrec)] if args.natoms else SUITE
    for natoms, nmeas, nrec in points:
        line = json.dumps(point(torch, ctx, natoms, nmeas, nrec, args.reps, args.chunk_gb, args.skip_torch))
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as fh:
                fh.write(line + "\n")


if __name__ == "__main__":
    main()

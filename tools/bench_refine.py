"""The Gauss-Newton step off the grid on the device (epgx_signal_refine: refine_kernel, csrc/epgx_refine.hip) against the routes
without it: a torch route on the same GPU (index_select of the atoms' columns, einsum for the accumulators, batched
linalg.solve), and downloading dictionary and Jacobian to run match.refine_host.

Workload: seeded complex Gaussian records [nrec][1 + P][natoms] (row 0 the dictionary, P derivative rows), signals
[nrec][nmeas] and uniformly random atoms, generated on the device (torch); nothing is simulated.  The library reads torch's buffers
through their addresses.  Device events around whole calls, one warm-up call each, `--reps` calls each, alternating; median, min
and max.  The host route is timed with the wall clock, once, and only where the records are at most --host-gb GB.

One JSON line per point:
  fused_ms, useful_bytes = (2 + P) * 16 * nrec * nmeas, fused_bytes_per_s, fused_share_of_hbm_peak (of 8 TB/s)
  torch_ms, speedup = torch_ms / fused_ms, agree = max |delta_fused - delta_torch| / max |delta_torch|
  host_download_ms, host_ms (where measured)

    python tools/bench_refine.py                          # natoms = 10^6, P = 2, nmeas = 65 536, nrec = 16, 64, 1000
    python tools/bench_refine.py --natoms 65536 --nmeas 65536 --nrec 16 --nparam 2 [--reps 5] [--skip-torch] [--host-gb 1] [--out FILE]
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

HBM_PEAK = 8.0e12            # bytes/s

SUITE = [(1000000, 65536, 16, 2), (1000000, 65536, 64, 2), (1000000, 65536, 1000, 2)]


def torch_refine(torch, X, S, idx):
    """the unclipped step by gather + einsum + batched solve; X [nrec][1 + P][natoms], S [nrec][nmeas]"""
    G = X.index_select(2, idx)                                            # [nrec, 1 + P, nmeas] through HBM
    d, j = G[:, 0], G[:, 1:]
    n = (d.real ** 2 + d.imag ** 2).sum(dim=0)
    c = (d.conj() * S).sum(dim=0)
    b = torch.einsum("tpm,tm->mp", j.conj(), S)
    h = torch.einsum("tm,tpm->mp", d.conj(), j)
    M = torch.einsum("tpm,tqm->mpq", j.conj(), j).real
    rho = c / n
    rho2 = rho.real ** 2 + rho.imag ** 2
    N = rho2[:, None, None] * (M - (h.conj()[:, :, None] * h[:, None, :]).real / n[:, None, None])
    y = (rho.conj()[:, None] * (b - rho[:, None] * h.conj())).real
    return torch.linalg.solve(N, y)


def stats(values):
    return dict(median=float(np.median(values)), min=float(np.min(values)), max=float(np.max(values)))


def point(torch, ctx, natoms, nmeas, nrec, P, reps, skip_torch, host_gb, seed=0):
    dev = torch.device("cuda", ctx.device)
    gen = torch.Generator(device=dev)
    gen.manual_seed(seed)
    X = torch.empty((nrec, 1 + P, natoms), dtype=torch.complex128, device=dev)
    for t in range(nrec):                                                 # (record by record: no second copy of a large buffer)
        X[t] = torch.view_as_complex(torch.randn((1 + P, natoms, 2), dtype=torch.float64, device=dev, generator=gen))
    S = torch.view_as_complex(torch.randn((nrec, nmeas, 2), dtype=torch.float64, device=dev, generator=gen))
    idx = torch.randint(0, natoms, (nmeas,), dtype=torch.int64, device=dev, generator=gen)
    torch.cuda.synchronize(dev)
    out = _lib.DeviceBuffer(ctx, (24 + 8 * P) * nmeas, itemsize=8)
    rows = np.arange(1, 1 + P, dtype=np.int32)
    V = ctypes.c_void_p

    def run_fused():
        _lib.check(ctx.lib.epgx_signal_refine(ctx.handle, V(X.data_ptr()), (1 + P) * natoms, natoms, 1 + P, nrec, P, rows.ctypes.data, natoms,
                                              V(S.data_ptr()), nmeas, nmeas, V(idx.data_ptr()), None, 1e-10, V(out.ptr.value + 16 * nmeas),
                                              out.ptr, V(out.ptr.value + (16 + 8 * P) * nmeas)), "epgx_signal_refine")

    def timed(fn):
        ctx.timer_start()
        fn()
        return ctx.timer_stop()

    run_fused()
    ctx.synchronize()
    fused_ms, torch_ms, tdelta = [], [], None
    if not skip_torch:
        tdelta = torch_refine(torch, X, S, idx)                           # warm-up
        torch.cuda.synchronize(dev)
    for _ in range(reps):                                                 # alternating
        fused_ms.append(timed(run_fused))
        if not skip_torch:
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            tdelta = torch_refine(torch, X, S, idx)
            t1.record()
            torch.cuda.synchronize(dev)
            torch_ms.append(t0.elapsed_time(t1))
    useful = (2 + P) * 16 * nrec * nmeas
    f = stats(fused_ms)
    res = dict(natoms=natoms, nmeas=nmeas, nrec=nrec, nparam=P, reps=reps, slices=_lib.refine_slices(nrec),
               fused_ms=f["median"], fused_ms_min=f["min"], fused_ms_max=f["max"], useful_bytes=useful,
               fused_bytes_per_s=useful / (f["median"] * 1e-3), fused_share_of_hbm_peak=useful / (f["median"] * 1e-3) / HBM_PEAK)
    delta = out.download(np.float64, ((3 + P) * nmeas,))[2 * nmeas:(2 + P) * nmeas].reshape(P, nmeas).T
    if not skip_torch:
        t = stats(torch_ms)
        want = tdelta.cpu().numpy()
        res.update(torch_ms=t["median"], torch_ms_min=t["min"], torch_ms_max=t["max"], speedup=t["median"] / f["median"],
                   agree=float(np.nanmax(np.abs(delta - want)) / np.max(np.abs(want))))
    if X.numel() * 16 <= host_gb * 1e9:
        t0 = time.perf_counter()
        host = X.cpu().numpy()
        t1 = time.perf_counter()
        ref = match.refine_host(host[:, 0], np.moveaxis(host[:, 1:], 1, 2), S.cpu().numpy(), idx.cpu().numpy())
        t2 = time.perf_counter()
        res.update(host_download_ms=1e3 * (t1 - t0), host_ms=1e3 * (t2 - t1),
                   host_agree=float(np.nanmax(np.abs(delta - ref.delta)) / np.nanmax(np.abs(ref.delta))))
    out.free()
    del X, S
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--natoms", type=int, default=0)
    ap.add_argument("--nmeas", type=int, default=65536)
    ap.add_argument("--nrec", type=int, default=16)
    ap.add_argument("--nparam", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-torch", action="store_true")
    ap.add_argument("--host-gb", type=float, default=1.0)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_refine: no GPU visible; this tool measures on the device only")
    ctx = _lib.get_context(0)
    points = [(args.natoms, args.nmeas, args.nrec, args.nparam)] if args.natoms else SUITE
    for natoms, nmeas, nrec, P in points:
        line = json.dumps(point(torch, ctx, natoms, nmeas, nrec, P, args.reps, args.skip_torch, args.host_gb))
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as fh:
                fh.write(line + "\n")


if __name__ == "__main__":
    main()

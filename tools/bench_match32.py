"""Single-precision dictionary matching (epgx_signal_match_c64: match32_kernel + match32_merge_kernel, csrc/epgx_match32.hip)
against the complex128 call (epgx_signal_match: match_kernel + match_merge_kernel) on the same GPU, in one process, alternating.

Workload and timing as tools/bench_match.py: seeded complex Gaussian dictionary [nrec][natoms] and signals [nrec][nmeas] generated
on the device (torch), read through their addresses; the complex64 operands are those buffers rounded once on the device
(epgx_signal_narrow, timed on its own).  Device events around whole calls, one warm-up call each, `--reps` calls each, alternating;
median, min and max.

One JSON line per point:
  pairs                    natoms * nmeas
  c128_ms, c64_ms          epgx_signal_match, epgx_signal_match_c64 (norms excluded: once per dictionary; *_norms_ms next to them)
  c128_pairs_per_s, c64_pairs_per_s
  c64_flops, c64_share_of_fp32_peak      8 * nrec flop per pair over c64_ms, over 157.3e12; c128_share_of_fp64_peak over 78.6e12
  ratio                    c128_ms / c64_ms  (above 1: the complex64 call is faster)
  narrow_dict_ms           rounding the dictionary (once per dictionary), narrow_sig_ms the signals (once per call of match.match)
  dict_bytes_c128, dict_bytes_c64
  agree                    share of voxels where both return the same atom (Gaussian data: far apart at either precision)

    python tools/bench_match32.py                         # the suite of DESIGN 4.13
    python tools/bench_match32.py --natoms 65536 --nmeas 65536 --nrec 16 [--reps 3] [--out FILE]
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
FP32_PEAK = 157.3e12         # flop/s, v_mfma_f32_16x16x4_f32 / v_mfma_f32_32x32x2_f32 = the fp32 vector rate

SUITE = [(1000000, 65536, 16), (1000000, 65536, 64), (1000000, 8192, 1000)]


def stats(values):
    return dict(median=float(np.median(values)), min=float(np.min(values)), max=float(np.max(values)))


def point(torch, ctx, natoms, nmeas, nrec, reps, seed=0):
    dev = torch.device("cuda", ctx.device)
    gen = torch.Generator(device=dev)
    gen.manual_seed(seed)
    D = torch.view_as_complex(torch.randn((nrec, natoms, 2), dtype=torch.float64, device=dev, generator=gen))
    S = torch.view_as_complex(torch.randn((nrec, nmeas, 2), dtype=torch.float64, device=dev, generator=gen))
    torch.cuda.synchronize(dev)
    D32 = _lib.DeviceBuffer(ctx, 8 * nrec * natoms, itemsize=8)
    S32 = _lib.DeviceBuffer(ctx, 8 * nrec * nmeas, itemsize=8)
    norms = _lib.DeviceBuffer(ctx, 8 * natoms, itemsize=8)
    norms32 = _lib.DeviceBuffer(ctx, 8 * natoms, itemsize=8)
    out = _lib.DeviceBuffer(ctx, 32 * nmeas, itemsize=8)
    out32 = _lib.DeviceBuffer(ctx, 32 * nmeas, itemsize=8)
    P = ctypes.c_void_p
    lib, h = ctx.lib, ctx.handle

    def narrow_dict():
        _lib.signal_narrow_into(ctx, D.data_ptr(), natoms, D32.ptr.value, natoms, nrec, natoms)

    def narrow_sig():
        _lib.signal_narrow_into(ctx, S.data_ptr(), nmeas, S32.ptr.value, nmeas, nrec, nmeas)

    def run_norms():
        _lib.check(lib.epgx_signal_norms(h, P(D.data_ptr()), natoms, nrec, natoms, norms.ptr), "epgx_signal_norms")

    def run_norms32():
        _lib.check(lib.epgx_signal_norms_c64(h, D32.ptr, natoms, nrec, natoms, norms32.ptr), "epgx_signal_norms_c64")

    def run128():
        _lib.check(lib.epgx_signal_match(h, P(D.data_ptr()), natoms, norms.ptr, natoms, P(S.data_ptr()), nmeas, nrec, nmeas, 0,
                                         P(out.ptr.value + 16 * nmeas), out.ptr, P(out.ptr.value + 24 * nmeas)), "epgx_signal_match")

    def run32():
        _lib.check(lib.epgx_signal_match_c64(h, D32.ptr, natoms, norms32.ptr, natoms, S32.ptr, nmeas, nrec, nmeas, 0,
                                             P(out32.ptr.value + 16 * nmeas), out32.ptr, P(out32.ptr.value + 24 * nmeas)),
                   "epgx_signal_match_c64")

    def timed(fn):
        ctx.timer_start()
        fn()
        return ctx.timer_stop()

    for fn in (narrow_dict, narrow_sig, run_norms, run_norms32, run128, run32):      # warm-up, and the operands of the timed calls
        fn()
    ctx.synchronize()
    nd = [timed(narrow_dict) for _ in range(reps)]
    ns = [timed(narrow_sig) for _ in range(reps)]
    n128 = [timed(run_norms) for _ in range(reps)]
    n32 = [timed(run_norms32) for _ in range(reps)]
    ms128, ms32 = [], []
    for _ in range(reps):                                                            # alternating
        ms128.append(timed(run128))
        ms32.append(timed(run32))
    i128 = out.download(np.float64, (4 * nmeas,))[2 * nmeas:3 * nmeas].view(np.int64)
    i32 = out32.download(np.float64, (4 * nmeas,))[2 * nmeas:3 * nmeas].view(np.int64)
    pairs = natoms * nmeas
    flop = 8.0 * nrec * pairs
    a, b = stats(ms128), stats(ms32)
    res = dict(natoms=natoms, nmeas=nmeas, nrec=nrec, pairs=pairs, reps=reps,
               c128_ms=a["median"], c128_ms_min=a["min"], c128_ms_max=a["max"], c64_ms=b["median"], c64_ms_min=b["min"], c64_ms_max=b["max"],
               c128_pairs_per_s=pairs / (a["median"] * 1e-3), c64_pairs_per_s=pairs / (b["median"] * 1e-3),
               c64_flops=flop / (b["median"] * 1e-3), c64_share_of_fp32_peak=flop / (b["median"] * 1e-3) / FP32_PEAK,
               c128_share_of_fp64_peak=flop / (a["median"] * 1e-3) / FP64_PEAK, ratio=a["median"] / b["median"],
               c128_norms_ms=stats(n128)["median"], c64_norms_ms=stats(n32)["median"],
               narrow_dict_ms=stats(nd)["median"], narrow_sig_ms=stats(ns)["median"],
               dict_bytes_c128=16 * nrec * natoms, dict_bytes_c64=8 * nrec * natoms, agree=float(np.mean(i128 == i32)))
    for buf in (D32, S32, norms, norms32, out, out32):
        buf.free()
    del D, S
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--natoms", type=int, default=0)
    ap.add_argument("--nmeas", type=int, default=65536)
    ap.add_argument("--nrec", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_match32: no GPU visible; this tool measures on the device only")
    ctx = _lib.get_context(0)
    points = [(args.natoms, args.nmeas, args.nrec)] if args.natoms else SUITE
    for natoms, nmeas, nrec in points:
        line = json.dumps(point(torch, ctx, natoms, nmeas, nrec, args.reps))
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as fh:
                fh.write(line + "\n")


if __name__ == "__main__":
    main()

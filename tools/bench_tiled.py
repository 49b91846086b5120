"""The tiled path for state matrices of any length (csrc/epgx_tiled.hip): one JSON line per leg.

    mrf3000   a 3000-TR unbounded FISP-MRF train over --nvox voxels on the tiled path: ms per call, launches, tile launches
    hyper2048 the 2048-order hyper-echo (2 x 511 echoes: up to 2046 orders) on run_split_kernel (today's path for it) and on
              the tiled entry called directly, same plan, same box
    mse511    a 511-echo train on run_contig_grow_kernel (1024 orders) and on the tiled entry: the price of the tiling

Executed fp64 flop come from the hardware counters of a separate `rocprofv3 --pmc` pass (the project's method, see
tools/collect_profiles.py): 64 lanes x (2 SQ_INSTS_VALU_FMA_F64 + SQ_INSTS_VALU_MUL_F64 + SQ_INSTS_VALU_ADD_F64) summed over
the tiled launches of ONE call; `share_fp64_peak` = that / time / 78.6 TFLOP/s.  Two steps on an MI355X:

    rocprofv3 --pmc SQ_INSTS_VALU_FMA_F64 SQ_INSTS_VALU_MUL_F64 SQ_INSTS_VALU_ADD_F64 --output-format csv -d OUT -- \
        python tools/bench_tiled.py --steps 1 --warmup 0 --legs mrf3000
    python tools/bench_tiled.py --legs mrf3000 --pmc OUT/*/*_counter_collection.csv
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from epgpy_amd import epg, _lib, functions, workloads  # noqa: E402

PEAK_FP64 = 78.6e12


def timed(ctx, fn, steps, warmup):
    for _ in range(warmup):
        fn()
    ctx.synchronize()
    ctx.timer_start()
    for _ in range(steps):
        fn()
    return ctx.timer_stop() / steps


def mrf_train(ntr, T1, T2):
    flips = 10 + 60 * np.abs(np.sin(np.arange(ntr) * np.pi / 500))
    seq = [epg.T(180, 0), epg.E(20, T1, T2), epg.SPOILER]
    for i, fa in enumerate(flips):
        seq += [epg.T(float(fa), 90.0 if i % 2 else 0.0), epg.E(2, T1, T2), epg.ADC, epg.E(8, T1, T2), epg.S(1)]
    return seq


def hyper_echo(npulse):
    echo1 = [epg.S(1), epg.T(10, 0), epg.S(1), epg.ADC]
    echo2 = [epg.S(1), epg.T(-10, 0), epg.S(1), epg.ADC]
    return [epg.T(90, 90)] + echo1 * npulse + [epg.S(1), epg.T(180, 0), epg.S(1)] + echo2 * npulse


def pmc_flop(path):
    """executed fp64 flop of the tiled kernels in a rocprofv3 --pmc counter CSV (of one call)"""
    import csv
    per = {"SQ_INSTS_VALU_FMA_F64": 2.0, "SQ_INSTS_VALU_MUL_F64": 1.0, "SQ_INSTS_VALU_ADD_F64": 1.0}
    total = 0.0
    with open(path) as fh:
        for r in csv.DictReader(fh):
            if "tiled_kernel" in r["Kernel_Name"] and r["Counter_Name"] in per:
                total += 64.0 * per[r["Counter_Name"]] * float(r["Counter_Value"])
    return total


def leg(ctx, name, seq, steps, warmup, K=None, pmc=None):
    """the tiled entry on `seq` (and, given K, epgx_run at K on the same plan)"""
    enc, _, _ = functions.compile_sequence(seq)
    Kbuf = enc.tiled_capacity()
    plan = enc.device_plan(ctx)
    nv = enc.nvox
    sig = _lib.DeviceBuffer(ctx, 16 * enc.n_adc * nv)
    info = _lib.tiled_info(ctx, plan, Kbuf)
    ms = timed(ctx, lambda: _lib.run_tiled(ctx, plan, 0, nv, None, Kbuf, sig.ptr.value, nv, 0), steps, warmup)
    out = {"leg": name, "nvox": nv, "Kbuf": Kbuf, "tiled_ms": round(ms, 3), "launches": info["blocks"] + info["shifts"],
           "tile_launches": info["tile_launches"], "kernels": info["names"]}
    if pmc is not None:
        flop = pmc_flop(pmc)
        out.update({"executed_tflop_per_call": round(flop / 1e12, 3), "share_fp64_peak": round(flop / (ms * 1e-3) / PEAK_FP64, 3),
                    "flop_source": "rocprofv3 --pmc SQ_INSTS_VALU_{FMA,MUL,ADD}_F64"})
    if K is not None:
        kname = _lib.kernel_for(ctx, plan, K)
        ms_ref = timed(ctx, lambda: _lib.run(ctx, plan, 0, plan.n_ops, 0, nv, None, None, K, sig.ptr.value, nv, 0), steps, warmup)
        out.update({"ref_kernel": kname, "ref_ms": round(ms_ref, 3), "tiled_over_ref": round(ms / ms_ref, 3)})
    sig.free()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nvox", type=int, default=16384)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--legs", nargs="*", default=["mrf3000", "hyper2048", "mse511"])
    ap.add_argument("--pmc", help="counter CSV of a rocprofv3 --pmc pass over ONE call of the mrf3000 leg (--steps 1 --warmup 0)")
    args = ap.parse_args()
    ctx = _lib.get_context(None)
    side = int(round(args.nvox ** 0.5))
    T1, T2 = np.linspace(200, 3000, side)[:, None], np.linspace(20, 300, args.nvox // side)[None, :]
    if "mrf3000" in args.legs:
        leg(ctx, "mrf3000", mrf_train(3000, T1, T2), args.steps, args.warmup, pmc=args.pmc)
    if "hyper2048" in args.legs:
        g = np.ones(args.nvox)      # (a grid of identical voxels: the plan has no per-voxel table)
        leg(ctx, "hyper2048", hyper_echo(511) + [epg.PD(g, reset=False)], args.steps, args.warmup, K=2048)
    if "mse511" in args.legs:
        leg(ctx, "mse511", workloads.mse_sequence(epg, T1, T2, necho=511), args.steps, args.warmup, K=1024)


if __name__ == "__main__":
    main()

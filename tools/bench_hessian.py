"""A Hessian over (tissue parameter x design variable) pairs: the fused passes (simulate(mode="resident"), one launch of
hess_kernel per pair) against the operator-by-operator path (mode="stepwise") on the same sequence.

Workload: a 20-echo multi-spin-echo train over an n x n (T1, T2) grid, every refocusing angle a design variable, the tissue
parameters T1, T2, B1: 3 x 20 pairs, K = 64.  One JSON line: the median wall time of `--reps` calls per mode after a warm-up
call (the whole call: compiling the passes, launches, download), and the largest relative difference between the two results.

    python tools/bench_hessian.py [--n 256] [--necho 20] [--reps 5] [--out profiles/hessian_bench.jsonl]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from epgpy_amd import epg, _lib  # noqa: E402


def workload(n, necho):
    T1 = np.linspace(300, 2500, n)[:, None]
    T2 = np.linspace(30, 250, n)[None, :]
    names = [f"a{i}" for i in range(necho)]
    tissue = ["T1", "T2", "B1"]
    rlx = epg.E(5.0, T1, T2, order1=["T1", "T2"], order2=[(t, a) for t in ("T1", "T2") for a in names])
    seq = [epg.T(90, 90, order1={"B1": {"alpha": 90.0}}, order2=[("B1", a) for a in names])]
    for a in names:
        rf = epg.T(150.0, 0, order1={"B1": {"alpha": 150.0}, a: {"alpha": 1.0}}, order2=[(t, a) for t in tissue] + [("B1", b) for b in names if b != a])
        seq += [epg.S(1), rlx, rf, epg.S(1), rlx, epg.ADC]
    return seq, epg.Hessian(tissue, names)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--necho", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    seq, probe = workload(args.n, args.necho)
    ctx = _lib.get_context(0)
    result, times = {}, {}
    for mode in ("resident", "stepwise"):
        result[mode] = epg.simulate(seq, probe=probe, mode=mode, max_nstate=63)       # warm-up
        laps = []
        for _ in range(args.reps):
            ctx.synchronize()
            t0 = time.perf_counter()
            epg.simulate(seq, probe=probe, mode=mode, max_nstate=63)
            ctx.synchronize()
            laps.append((time.perf_counter() - t0) * 1e3)
        times[mode] = float(np.median(laps))
        print(mode, [round(x, 1) for x in laps], flush=True)
    scale = np.max(np.abs(result["stepwise"]), axis=tuple(range(result["stepwise"].ndim - 2)))
    diff = np.max(np.abs(result["resident"] - result["stepwise"]), axis=tuple(range(result["stepwise"].ndim - 2)))
    line = dict(workload=f"{args.necho}-echo MSE, 3 x {args.necho} pairs, {args.n} x {args.n} voxels, K = 64", reps=args.reps,
                resident_ms=times["resident"], stepwise_ms=times["stepwise"], ratio=times["stepwise"] / times["resident"],
                max_rel_diff=float(np.max(diff / np.where(scale > 0, scale, 1.0))))
    print(json.dumps(line))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as fh:
            fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
